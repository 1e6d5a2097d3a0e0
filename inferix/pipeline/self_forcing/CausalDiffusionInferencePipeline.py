"""inferix/pipeline/self_forcing/CausalDiffusionInferencePipeline.py:10 -> inferix_amd.pipeline.causal_diffusion_inference"""
from inferix_amd.pipeline.causal_diffusion_inference import CausalDiffusionInferencePipeline  # noqa: F401
