"""reference pcseg/model/segmentor/range/fidnet/model"""
