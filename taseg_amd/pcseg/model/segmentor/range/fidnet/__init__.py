"""FIDNet (reference pcseg/model/segmentor/range/fidnet)."""
