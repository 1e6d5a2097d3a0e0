from .base_pipeline import AbstractInferencePipeline
from .causal_diffusion_inference import CausalDiffusionInferencePipeline
from .causal_inference import CausalInferencePipeline
from .causvid import CausVidPipeline
from .causvid_inference import CausVidInferencePipeline
from .magi import MagiPipeline
from .self_forcing import SelfForcingPipeline

__all__ = ["AbstractInferencePipeline", "CausalDiffusionInferencePipeline", "CausalInferencePipeline", "CausVidInferencePipeline", "CausVidPipeline", "MagiPipeline",
           "SelfForcingPipeline"]
