"""CENet (reference pcseg/model/segmentor/range/cenet)."""
