"""reference pcseg/model/segmentor/range/salsanext/model"""
