"""``model.aagcn_v24`` -- the class path the reference aagcn_v24 configs name (train_joint_aagcn_v24.yaml:34).
The implementation lives in ``2s-agcn_amd/model/aagcn_v24.py``."""
import agcn_amd  # noqa: F401
from agcn_amd.model.aagcn_v24 import (CosSinPositionalEncoding, Model, PositionalEncoding,  # noqa: F401
                                      TransformerEncoderExt, TransformerEncoderLayerExt,
                                      TransformerEncoderLayerExtV2, transformer_config_checker)
