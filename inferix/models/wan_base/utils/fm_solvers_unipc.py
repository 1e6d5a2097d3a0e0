"""inferix/models/wan_base/utils/fm_solvers_unipc.py:23 -> inferix_amd.schedulers.FlowUniPCSchedule (the part of the class the
many-step causal sampler uses: set_timesteps, timesteps, sigmas, step)"""
from inferix_amd.schedulers import FlowUniPCSchedule  # noqa: F401

FlowUniPCMultistepScheduler = FlowUniPCSchedule
