"""Kernel time of the top-k retrieval against the rank kernel and torch on the same operands, one GPU, one JSON line:

    python tools/bench_retrieval.py [ROUNDS]

Two problems, fp32 normalised rows, k = 10: "large" (a gallery of 65,536 x 512, 4,096 queries) and "cmu" (a CMU-MOSEI evaluation
split queried against itself: the width is ``hidden_size`` of configs/CMU_config1.yaml over the training defaults; configs/ holds no
row count and the dataset is not in the tree, so the rows are the public test split's 4,659).  Per problem three times in
microseconds, each the median over ROUNDS (30) launches between device events after 5 warm-up rounds, the three launches
alternating inside every round of one process:
  topk_us   mca_cosine_topk_f32 (both launches: the chunk kernel and the merge);
  rank_us   mca_cosine_rank_f32 on the same operands (query r's true target is target r);
  torch_us  torch's fp32 (q @ t.T).topk(k), which stores the (queries, gallery) matrix.
identity_ok: rank[r] < k  <=>  s_true[r] >= score[r][k - 1] held for every query (the two kernels share one fmaf chain)."""
import importlib
import json
import os
import sys
import time

import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.bench_lp import _peak_sclk_mhz          # noqa: E402

CMU_TEST_ROWS = 4659          # CMU-MOSEI's standard test split (Zadeh et al. 2018, the SDK's standard folds)
K = 10


def problems(P):
    cfg = P.config.default_train_config()
    with open(os.path.join(REPO, "configs", "CMU_config1.yaml")) as f:
        cfg.update(yaml.safe_load(f) or {})
    return {"large": (4096, 65536, 512), "cmu": (CMU_TEST_ROWS, CMU_TEST_ROWS, int(cfg["hidden_size"]))}


def main():
    importlib.import_module("mca-paper_amd.build").build(verbose=False)
    P = importlib.import_module("mca-paper_amd")
    H = importlib.import_module("mca-paper_amd.hip")
    M = importlib.import_module("mca-paper_amd.metrics")
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval.py measures on a HIP device and none is available")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(11)
    rec = {"what": "bench_retrieval", "device": torch.cuda.get_device_name(0), "sclk_mhz_max": _peak_sclk_mhz(0), "k": K, "rounds": rounds}
    for tag, (nq, nt, d) in problems(P).items():
        q = M.normalize_rows(torch.randn(nq, d, device=dev, generator=g))
        t = M.normalize_rows(torch.randn(nt, d, device=dev, generator=g))
        ws = torch.empty(H.lib().mca_cosine_topk_workspace(nq, nt, K), dtype=torch.uint8, device=dev)
        score, index = torch.empty(nq, K, device=dev), torch.empty(nq, K, dtype=torch.int32, device=dev)
        s_true, rank = torch.empty(nq, device=dev), torch.empty(nq, dtype=torch.int32, device=dev)
        kept = {}

        def topk():
            H.call("mca_cosine_topk_f32", q.data_ptr(), d, None, nq, t.data_ptr(), d, nt, d, None, None, K, ws.data_ptr(), ws.numel(),
                   score.data_ptr(), K, index.data_ptr(), K, H.stream_ptr())

        def rank_():
            H.call("mca_cosine_rank_f32", q.data_ptr(), d, None, nq, t.data_ptr(), d, nt, d, s_true.data_ptr(), rank.data_ptr(), H.stream_ptr())

        def torch_():
            kept["torch"] = (q @ t.T).topk(K)

        fns = (("topk", topk), ("rank", rank_), ("torch", torch_))
        for _ in range(5):
            for _, fn in fns:
                fn()
        torch.cuda.synchronize()
        evs = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)] for k, _ in fns}
        for i in range(rounds):
            for k, fn in fns:
                s, e = evs[k][i]
                s.record(); fn(); e.record()
        torch.cuda.synchronize()
        for k, lst in evs.items():
            ts = sorted(s.elapsed_time(e) for s, e in lst)
            rec[f"{tag}_{k}_us"] = round(ts[len(ts) // 2] * 1e3, 1)
            rec[f"{tag}_{k}_us_min_max"] = [round(ts[0] * 1e3, 1), round(ts[-1] * 1e3, 1)]
        rec[f"{tag}_shape"] = f"queries={nq} gallery={nt} d={d}"
        rec[f"{tag}_topk_over_rank"] = round(rec[f"{tag}_topk_us"] / rec[f"{tag}_rank_us"], 3)
        rec[f"{tag}_workspace_mib"] = round(ws.numel() / 2 ** 20, 2)
        rec[f"{tag}_identity_ok"] = bool(torch.equal(rank < K, s_true >= score[:, K - 1]))
        rec[f"{tag}_index_equals_torch"] = round(float((index.long() == kept["torch"].indices).float().mean()), 6)          # torch's matmul rounds differently
        del kept, q, t, ws
    rec["utc"] = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
