"""Graph construction on the GPU (mirror of ``RCAEval/graph_construction``)."""
from .lingam import DirectLiNGAM  # noqa: E402,F401
