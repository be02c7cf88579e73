"""Point-voxel fusion segmentors (reference pcseg/model/segmentor/fusion): SPVCNN.  RPVNet is not built."""
