"""Mixture-of-experts layers -- module paths of ``llm_quest/moe/``.  Built here: ``qwen3_moe`` (Qwen3 / Qwen3-Next routing without the shared
expert), ``deepseek_moe`` (DeepSeekMoE) and ``nvidia_latent_moe`` (Nemotron-3 LatentMoE).  The classic variant is out of scope."""
