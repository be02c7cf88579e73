"""reference pcseg/model/segmentor/range/cenet/model"""
