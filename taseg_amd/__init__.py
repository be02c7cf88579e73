"""taseg_amd - MI355X-native (gfx950, HIP) implementation of the TASeg / OpenPCSeg hot path:
voxelisation -> sparse-conv MinkUNet backbone -> multi-scan temporal aggregation.

  taseg_amd.backend       torch-facing wrappers of the C ABI (include/taseg_hip.h)
  taseg_amd.torchsparse   torchsparse v1.4.0-compatible operator API on that backend
  taseg_amd.pcseg         pcseg.model-compatible segmentors (MinkUNet, MinkUNetMs, build_network), pcseg.loss, pcseg.optim
  taseg_amd.data          synthetic SemanticKITTI-shaped scans + the device data stage
"""
import sys

__version__ = "0.1.0"


def install_as_dropin():
    """Register the compatible packages under the reference's import names so unmodified
    OpenPCSeg code (`import torchsparse`, `from pcseg.model import build_network`, `from pcseg.optim import build_optimizer`)
    binds to them."""
    from . import torchsparse as ts
    from . import pcseg as pc
    from .pcseg.model import segmentor as seg
    from .pcseg.model.segmentor import fusion
    from .pcseg.model.segmentor.fusion import rpvnet, spvcnn
    from .pcseg.model.segmentor import range as range_view
    from .pcseg.model.segmentor.range import utils as range_utils
    from .pcseg.model.segmentor.range import salsanext as sn
    from .pcseg.model.segmentor.range.salsanext import model as sn_model
    from .pcseg.model.segmentor.range.salsanext.model import semantic as sn_semantic
    from .pcseg.model.segmentor.range.salsanext.model.semantic import salsanext as sn_file
    from .pcseg.model.segmentor.range import cenet, fidnet
    from .pcseg.model.segmentor.range.cenet import model as ce_model
    from .pcseg.model.segmentor.range.cenet.model import semantic as ce_semantic
    from .pcseg.model.segmentor.range.cenet.model.semantic import cenet as ce_file
    from .pcseg.model.segmentor.range.fidnet import model as fid_model
    from .pcseg.model.segmentor.range.fidnet.model import semantic as fid_semantic
    from .pcseg.model.segmentor.range.fidnet.model.semantic import fidnet as fid_file
    names = {"torchsparse": ts, "torchsparse.nn": ts.nn, "torchsparse.nn.functional": ts.nn.functional,
             "torchsparse.nn.utils": ts.nn.utils, "torchsparse.utils": ts.utils,
             "torchsparse.utils.quantize": ts.utils.quantize, "torchsparse.utils.collate": ts.utils.collate,
             "torchsparse.backend": ts.backend, "torchsparse.tensor": ts.tensor,
             "pcseg": pc, "pcseg.model": pc.model, "pcseg.loss": pc.loss, "pcseg.optim": pc.optim,
             # (SPVCNN and RPVNet are reached by the reference's module path, not by the registry: pcseg/model/segmentor/__init__.py)
             "pcseg.model.segmentor": seg, "pcseg.model.segmentor.fusion": fusion, "pcseg.model.segmentor.fusion.spvcnn": spvcnn,
             "pcseg.model.segmentor.fusion.rpvnet": rpvnet,
             # (SalsaNext and the range-view family's losses and kNN post-processing: by the reference's module path, like the two above)
             "pcseg.model.segmentor.range": range_view, "pcseg.model.segmentor.range.utils": range_utils,
             "pcseg.model.segmentor.range.salsanext": sn, "pcseg.model.segmentor.range.salsanext.model": sn_model,
             "pcseg.model.segmentor.range.salsanext.model.semantic": sn_semantic,
             "pcseg.model.segmentor.range.salsanext.model.semantic.salsanext": sn_file,
             # (FIDNet and CENet, the same way)
             "pcseg.model.segmentor.range.fidnet": fidnet, "pcseg.model.segmentor.range.fidnet.model": fid_model,
             "pcseg.model.segmentor.range.fidnet.model.semantic": fid_semantic,
             "pcseg.model.segmentor.range.fidnet.model.semantic.fidnet": fid_file,
             "pcseg.model.segmentor.range.cenet": cenet, "pcseg.model.segmentor.range.cenet.model": ce_model,
             "pcseg.model.segmentor.range.cenet.model.semantic": ce_semantic,
             "pcseg.model.segmentor.range.cenet.model.semantic.cenet": ce_file}
    for name, mod in names.items():
        sys.modules.setdefault(name, mod)
    return names
