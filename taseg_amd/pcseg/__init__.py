"""pcseg-compatible surface of the hot path: `pcseg.model.build_network`, the MinkUNet family
segmentors, the loss they call and the optimizer / scheduler builders of the training loop (reference: pcseg/{model,loss,optim})."""
from . import loss, model, optim  # noqa: F401
