"""Direct Preference Optimization on HIP kernels (reference: llm_quest/alignment/dpo)."""
