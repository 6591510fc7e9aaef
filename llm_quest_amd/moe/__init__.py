"""Mixture-of-experts layers -- module paths of ``llm_quest/moe/``.  Built here: ``qwen3_moe`` (Qwen3 / Qwen3-Next routing without the shared
expert).  The classic, DeepSeek and latent variants are out of scope."""
