"""``model.sgn_v15`` -- the class path the reference's v15 configs name (train_sgn_v15.yaml).
The implementation lives in ``2s-agcn_amd/model/sgn_v15.py``."""
import agcn_amd  # noqa: F401
from agcn_amd.model.sgn_v15 import SGN  # noqa: F401
