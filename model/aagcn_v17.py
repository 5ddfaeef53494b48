"""``model.aagcn_v17`` -- the class path the reference aagcn_v17 configs name (train_joint_aagcn_v17.yaml:35).
The implementation lives in ``2s-agcn_amd/model/aagcn_v17.py``."""
import agcn_amd  # noqa: F401
from agcn_amd.model.aagcn_v17 import (CosSinPositionalEncoding, Model, PositionalEncoding,  # noqa: F401
                                      TransformerEncoderLayerExt, generate_square_subsequent_mask)
