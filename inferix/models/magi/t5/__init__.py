"""inferix/models/magi/t5: `T5Embedder` (t5_model.py:27-150), the fp32 T5 v1.1 XXL caption encoder, on the HIP kernels.  The tokenizer
and the caption cleaning are handed in; checkpoint download is not built."""
from inferix_amd.magi.t5 import HipT5Embedder, HipT5v11Encoder  # noqa: F401

T5Embedder = HipT5Embedder

__all__ = ["T5Embedder", "HipT5Embedder", "HipT5v11Encoder"]
