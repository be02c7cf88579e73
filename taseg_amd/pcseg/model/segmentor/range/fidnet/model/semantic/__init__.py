"""reference pcseg/model/segmentor/range/fidnet/model/semantic"""
from .fidnet import FIDNet  # noqa: F401
