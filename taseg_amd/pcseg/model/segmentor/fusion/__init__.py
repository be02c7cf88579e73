"""Point-voxel fusion segmentors (reference pcseg/model/segmentor/fusion): SPVCNN and RPVNet (range-point-voxel)."""
