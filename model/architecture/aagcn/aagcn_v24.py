"""``model.architecture.aagcn.aagcn_v24`` -- the reference's own module path of aagcn_v24.
The implementation lives in ``2s-agcn_amd/model/aagcn_v24.py``."""
import agcn_amd  # noqa: F401
from agcn_amd.model.aagcn_v24 import (CosSinPositionalEncoding, Model, PositionalEncoding,  # noqa: F401
                                      TransformerEncoderExt, TransformerEncoderLayerExt,
                                      TransformerEncoderLayerExtV2, transformer_config_checker)
