"""inferix/pipeline/magi/pipeline.py:32 -> inferix_amd.pipeline.magi (the parts are injected: config object, dit, vae, embedder)"""
from inferix_amd.pipeline.magi import MagiPipeline  # noqa: F401
