from .rpvnet import RPVNet, SalsaNext  # noqa: F401
