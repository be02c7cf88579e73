"""reference pcseg/model/segmentor/range/salsanext/model/semantic"""
from .salsanext import SalsaNext  # noqa: F401
