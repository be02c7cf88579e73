from .synthetic import (AttrDict, FLEXIBLE_STEPS_KITTI, fill_parameters, make_model_cfg, synth_pose,  # noqa: F401
                        synth_scan)
from .cylinder import CylinderGrid, build_cylinder_batch, build_cylinder_tta_batch  # noqa: F401
