"""``model.architecture.aagcn.aagcn_v17`` -- the reference's own module path of aagcn_v17.
The implementation lives in ``2s-agcn_amd/model/aagcn_v17.py``."""
import agcn_amd  # noqa: F401
from agcn_amd.model.aagcn_v17 import (CosSinPositionalEncoding, Model, PositionalEncoding,  # noqa: F401
                                      TransformerEncoderLayerExt, generate_square_subsequent_mask)
