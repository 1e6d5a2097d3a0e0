"""inferix/models/wan_base/__init__.py: the names the Self-Forcing pipelines import from here"""
from .utils.fm_solvers_unipc import FlowUniPCMultistepScheduler  # noqa: F401
