"""Alignment (reference: llm_quest/alignment): the GRPO loss layer of ``rlhf_grpo``."""
