"""Alignment (reference: llm_quest/alignment): the GRPO loss layer and the reward model of ``rlhf_grpo``, DPO in ``dpo``."""
