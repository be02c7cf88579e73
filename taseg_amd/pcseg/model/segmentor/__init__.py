"""Segmentor registry (reference pcseg/model/segmentor/__init__.py:29-62).  The TASeg hot-path models and Cylinder_TS (the
network the anisotropic / overlapping-window convolutions were added for) exist here; the other OpenPCSeg backbones are out of
scope.

SPVCNN is built too (`fusion/spvcnn/`), but is not in this registry: it is constructed through the reference's module path,
`from pcseg.model.segmentor.fusion.spvcnn import SPVCNN; SPVCNN(model_cfgs, num_class)`, and `build_segmentor(NAME="SPVCNN")` keeps
raising NotImplementedError - two existing tests pin that and `_OUT_OF_SCOPE` as they stand (tests/test_spvcnn_host.py says which).
RPVNet (`fusion/rpvnet/`) is built and reached the same way, for the same reason, and so is SalsaNext
(`range/salsanext/model/semantic/salsanext.py`, with the range-view family's losses and kNN step in `range/utils.py`), FIDNet
(`range/fidnet/model/semantic/fidnet.py`) and CENet (`range/cenet/model/semantic/cenet.py`)."""
from .base_segmentors import BaseSegmentor
from .voxel.cylinder3d.cylinder_ts import Cylinder_TS
from .voxel.minkunet.minkunet import MinkUNet
from .voxel.minkunet.minkunet_ms import MinkUNetMs
from .voxel.minkunet.minkunet_ms_kd import MinkUNetMsKd
from .voxel.minkunet.minkunet_ms_mm import MinkUNetMsMm, MinkUNetMsMmNus

__all__ = {
    "MinkUNet": MinkUNet,
    "MinkUNetMs": MinkUNetMs,
    "MinkUNetMsKd": MinkUNetMsKd,
    "MinkUNetMsMm": MinkUNetMsMm,
    "MinkUNetMsMmNus": MinkUNetMsMmNus,
    "Cylinder_TS": Cylinder_TS,
}

_OUT_OF_SCOPE = ("RangeNet++", "SalsaNext", "FIDNet", "CENet", "SPVCNN", "RPVNet")


def build_segmentor(model_cfgs, num_class):
    name = model_cfgs.NAME
    if name not in __all__:
        if name in _OUT_OF_SCOPE:
            raise NotImplementedError(f"segmentor '{name}' is outside the TASeg hot path built here")
        raise NameError(f"name '{name}' is not defined")  # what the reference's eval(NAME) raises
    return __all__[name](model_cfgs=model_cfgs, num_class=num_class)
