import agcn_amd  # noqa: F401
from agcn_amd.online import (ActionRecognition, MultiStreamRecognition, RecordingRecognition,  # noqa: F401
                             load_model, window_plan)
