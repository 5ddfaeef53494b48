"""``model.sgn`` -- the class path the reference's SGN configs name (train_joint_aagcn_preprocess_sgn_model.yaml).
The implementation lives in ``2s-agcn_amd/model/sgn.py``."""
import agcn_amd  # noqa: F401
from agcn_amd.model.sgn import SGN  # noqa: F401
