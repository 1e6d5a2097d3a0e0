"""inferix/pipeline/magi/prompt_process.py: the special tokens and their env switches :31-92, pad_special_token :95-129 and
get_txt_embeddings :184-212 for one process (the embedder is handed in; the tensor-parallel broadcast is not built).  The special-token
file is read on first use (`load_special_tokens`), not at import."""
from inferix_amd.magi.prompt import (env_is_true, get_negative_special_token_keys, get_special_token_keys, get_txt_embeddings,  # noqa: F401
                                     load_special_tokens, pad_special_token)
from inferix_amd.magi.t5 import HipT5Embedder as T5Embedder  # noqa: F401
