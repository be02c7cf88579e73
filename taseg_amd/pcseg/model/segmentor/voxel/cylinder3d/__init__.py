from .cylinder_ts import Cylinder_TS  # noqa: F401
