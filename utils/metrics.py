"""``utils.metrics`` of the reference (utils/metrics.py:20-70): Wang-Isola alignment / uniformity accumulators, and the
retrieval rank metrics of the probe stage; beyond the reference, top-k retrieval and the kNN readout (retrieve_accel_gpu.py)."""
import importlib as _il

_m = _il.import_module("mca-paper_amd.metrics")
Alignment, Uniformity, lalign, lunif = _m.Alignment, _m.Uniformity, _m.lalign, _m.lunif
get_rank_metrics, get_rank, compute_cosines, uniformity = _m.get_rank_metrics, _m.get_rank, _m.compute_cosines, _m.uniformity          # :72-98
cosine_topk, knn_predict, hits_at = _m.cosine_topk, _m.knn_predict, _m.hits_at

__all__ = ["Alignment", "Uniformity", "lalign", "lunif", "get_rank_metrics", "get_rank", "compute_cosines", "uniformity",
           "cosine_topk", "knn_predict", "hits_at"]
