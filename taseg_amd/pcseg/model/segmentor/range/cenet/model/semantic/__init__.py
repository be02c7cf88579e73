"""reference pcseg/model/segmentor/range/cenet/model/semantic"""
from .cenet import CENet  # noqa: F401
