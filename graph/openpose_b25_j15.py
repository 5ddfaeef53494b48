import agcn_amd  # noqa: F401
from agcn_amd.graph.openpose_b25_j15 import *  # noqa: F401,F403
from agcn_amd.graph.openpose_b25_j15 import Graph  # noqa: F401
