"""Times the fused GEGLU GEMMs of one fusion layer at the step's shape (T = 2538 b rows, ip = 1408, D = 512; b = argv[1], default
32) in both forms: h = [a | gate] kept and gelu evaluated again in the backward (mca_gemm_nt_geglu_fwd / _bwd), against the saved
factors (mca_gemm_nt_geglu_fwd_saved / _bwd_saved).  One process, the two forms in alternating order, argv[2] pairs (default 5);
one line per pair and the summary profiles/geglu_saved_factors.md quotes."""
import importlib, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H = importlib.import_module("mca-paper_amd.hip"); H.lib()
b = int(sys.argv[1]) if len(sys.argv) > 1 else 32
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
T, D, Ip = b * 2538, 512, 1408
bf = lambda *s: torch.randn(*s, device="cuda").bfloat16()
empty = lambda *s: torch.empty(*s, device="cuda", dtype=torch.bfloat16)
x_b, w1, dxo, w2T = bf(T, D), bf(2 * Ip, D) * 0.05, bf(T, D), bf(Ip, D) * 0.05
h, g, dh = empty(T, 2 * Ip), empty(T, Ip), empty(T, 2 * Ip)
S = H.stream_ptr
fwd = lambda name: H.call(name, x_b.data_ptr(), D, w1.data_ptr(), D, h.data_ptr(), 2 * Ip, g.data_ptr(), Ip, Ip, T, D, S())
bwd = lambda name: H.call(name, dxo.data_ptr(), D, w2T.data_ptr(), D, h.data_ptr(), dh.data_ptr(), 2 * Ip, Ip, T, D, S())


def timed(fn, name, reps=20):
    for _ in range(3): fn(name)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): fn(name)
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


rows = []
for p in range(pairs):
    order = ("", "_saved") if p % 2 == 0 else ("_saved", "")
    t = {}
    for suffix in order:          # the backward reads what the forward of the same form left in h
        t["fwd" + suffix] = timed(fwd, "mca_gemm_nt_geglu_fwd" + suffix)
        t["bwd" + suffix] = timed(bwd, "mca_gemm_nt_geglu_bwd" + suffix)
    rows.append(t)
    print(f"pair {p}: fwd {t['fwd']:7.1f} -> saved {t['fwd_saved']:7.1f} us ({t['fwd_saved'] - t['fwd']:+6.1f})   "
          f"bwd {t['bwd']:7.1f} -> saved {t['bwd_saved']:7.1f} us ({t['bwd_saved'] - t['bwd']:+6.1f})   "
          f"net {t['fwd_saved'] + t['bwd_saved'] - t['fwd'] - t['bwd']:+6.1f} us", flush=True)
col = lambda k: [r[k] for r in rows]
for k in ("fwd", "fwd_saved", "bwd", "bwd_saved"):
    v = col(k)
    print(f"{k:10s} min {min(v):7.1f}  median {sorted(v)[len(v) // 2]:7.1f}  max {max(v):7.1f} us   (spread between pairs {max(v) - min(v):5.1f})")
net = [r["fwd_saved"] + r["bwd_saved"] - r["fwd"] - r["bwd"] for r in rows]
print(f"net per layer (saved - unsaved, fwd + bwd): min {min(net):+.1f}  median {sorted(net)[len(net) // 2]:+.1f}  max {max(net):+.1f} us")
