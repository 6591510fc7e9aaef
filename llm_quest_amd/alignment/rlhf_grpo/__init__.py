"""GRPO policy losses on HIP kernels (reference: llm_quest/alignment/rlhf_grpo)."""
