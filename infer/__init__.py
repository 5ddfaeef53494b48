"""Top-level ``infer`` package: keeps the reference's ``infer.inference.ActionRecognition`` resolvable."""
from . import inference  # noqa: F401
