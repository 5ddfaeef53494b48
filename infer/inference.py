import agcn_amd  # noqa: F401
from agcn_amd.online import ActionRecognition, load_model  # noqa: F401
