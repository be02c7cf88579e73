from .spvcnn import SPVCNN  # noqa: F401
