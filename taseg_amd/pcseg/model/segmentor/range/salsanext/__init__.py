"""SalsaNext (reference pcseg/model/segmentor/range/salsanext)."""
