"""Times the fused data-gradient GEMM + LayerNorm backward (mca_gemm_nt_res_lnbwd) against the pair of launches it replaces
(mca_gemm_nt with fp32 output and residual, then mca_layernorm_bwd) on the step's three shapes (T = 2538 b rows, D = 512; b =
argv[1], default 32): dh.W1 + dx (K = 2816), dqkv.Wqkv + dx (K = 1536) and the pooling's dkv.Wkv (K = 1024, no residual).  One
process, the two forms in alternating order, argv[2] pairs (default 5); one line per pair and shape, then the summary
profiles/ln_rows_fusion.md quotes.  Every repetition streams its own operands from HBM: the fused form works in place (dx is the
residual), the pair ping-pongs between two buffers as the engine does."""
import importlib, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H = importlib.import_module("mca-paper_amd.hip"); H.lib()
b = int(sys.argv[1]) if len(sys.argv) > 1 else 32
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
T, D = b * 2538, 512
SHAPES = [("dh.W1 + dx", 2816, True), ("dqkv.Wqkv + dx", 1536, True), ("dkv.Wkv", 1024, False)]
f32 = lambda *s: torch.randn(*s, device="cuda")
x, dxa, dxb = f32(T, D), f32(T, D), f32(T, D)
dx_b = torch.empty(T, D, device="cuda", dtype=torch.bfloat16)
gamma, dgamma = torch.rand(D, device="cuda") * 0.5 + 0.75, torch.zeros(D, device="cuda")
mean, rstd = x.mean(1).contiguous(), (1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)).contiguous()
S = H.stream_ptr


def launches(K, res):
    A, B = torch.randn(T, K, device="cuda").bfloat16(), (torch.randn(D, K, device="cuda") * K ** -0.5).bfloat16()
    r = dxa if res else None

    def pair():
        H.call("mca_gemm_nt", A.data_ptr(), K, B.data_ptr(), K, dxb.data_ptr(), D, 0, None, H.ptr(r), D if res else 0, 0, T, D, K, S())
        H.call("mca_layernorm_bwd", dxb.data_ptr(), D, 0, 0, x.data_ptr(), D, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None,
               dxa.data_ptr(), D, dx_b.data_ptr(), D, dgamma.data_ptr(), None, None, T, D, S())

    def fused():
        H.call("mca_gemm_nt_res_lnbwd", A.data_ptr(), K, B.data_ptr(), K, H.ptr(r), D if res else 0, x.data_ptr(), D, mean.data_ptr(),
               rstd.data_ptr(), gamma.data_ptr(), dxa.data_ptr(), D, dx_b.data_ptr(), D, dgamma.data_ptr(), T, D, K, S())
    return pair, fused


def timed(fn, reps=20):
    for _ in range(3): fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


rows = {name: [] for name, _, _ in SHAPES}
for name, K, res in SHAPES:
    pair, fused = launches(K, res)
    for p in range(pairs):
        t = {}
        for form in (("pair", "fused") if p % 2 == 0 else ("fused", "pair")):
            dxa.normal_()          # (the in-place form would otherwise feed its own output back 20 times)
            t[form] = timed(pair if form == "pair" else fused)
        rows[name].append(t)
        print(f"{name:16s} K={K:5d} pair {p}: two launches {t['pair']:7.1f} us -> fused {t['fused']:7.1f} us ({t['fused'] - t['pair']:+6.1f})", flush=True)
print(f"T = {T}, D = {D}; us per launch (pair: both launches together)")
for name, K, res in SHAPES:
    for form in ("pair", "fused"):
        v = sorted(r[form] for r in rows[name])
        print(f"{name:16s} K={K:5d} {form:5s} min {v[0]:7.1f}  median {v[len(v) // 2]:7.1f}  max {v[-1]:7.1f}   (spread between pairs {v[-1] - v[0]:5.1f})")
    d = sorted(r["fused"] - r["pair"] for r in rows[name])
    print(f"{name:16s} K={K:5d} fused - pair: min {d[0]:+.1f}  median {d[len(d) // 2]:+.1f}  max {d[-1]:+.1f} us")
