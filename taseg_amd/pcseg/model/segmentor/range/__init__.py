"""Range-view segmentors (reference pcseg/model/segmentor/range): the family's kNN post-processing (`utils.KNN`) on ts_rv_knn."""
