"""Times the two tile heights of the fused data-gradient GEMM + LayerNorm backward against each other: mca_gemm_nt_res_lnbwd (128
rows per workgroup) and mca_gemm_nt_res_lnbwd_tall with its 160-row kernel forced (knob 15 = 2), on the step's three shapes
(T = 2538 b rows, D = 512; b = argv[1], default 32): dh.W1 + dx (K = 2816), dqkv.Wqkv + dx (K = 1536) and the pooling's dkv.Wkv
(K = 1024, no residual).  One process, the two forms in alternating order, argv[2] pairs (default 5); one line per pair and shape,
then the summary profiles/ln_rows_tall.md quotes, with the height the rule of csrc/gemm_plan.h picks for this device beside it: a
shape must not be routed to a form that measures slower here.  Both forms work in place (dx is the residual), as in the engine."""
import ctypes as C, importlib, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H = importlib.import_module("mca-paper_amd.hip"); H.lib()
b = int(sys.argv[1]) if len(sys.argv) > 1 else 32
pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
T, D = b * 2538, 512
SHAPES = [("dh.W1 + dx", 2816, True), ("dqkv.Wqkv + dx", 1536, True), ("dkv.Wkv", 1024, False)]
FORMS = {"128": ("mca_gemm_nt_res_lnbwd", 0), "160": ("mca_gemm_nt_res_lnbwd_tall", 2)}          # entry point, knob 15
f32 = lambda *s: torch.randn(*s, device="cuda")
x, dxa = f32(T, D), f32(T, D)
dx_b = torch.empty(T, D, device="cuda", dtype=torch.bfloat16)
gamma, dgamma = torch.rand(D, device="cuda") * 0.5 + 0.75, torch.zeros(D, device="cuda")
mean, rstd = x.mean(1).contiguous(), (1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)).contiguous()
S = H.stream_ptr
cus = torch.cuda.get_device_properties(0).multi_processor_count


def launch(K, res):
    A, B = torch.randn(T, K, device="cuda").bfloat16(), (torch.randn(D, K, device="cuda") * K ** -0.5).bfloat16()
    r = dxa if res else None

    def fn(entry):
        H.call(entry, A.data_ptr(), K, B.data_ptr(), K, H.ptr(r), D if res else 0, x.data_ptr(), D, mean.data_ptr(),
               rstd.data_ptr(), gamma.data_ptr(), dxa.data_ptr(), D, dx_b.data_ptr(), D, dgamma.data_ptr(), T, D, K, S())
    return fn


def timed(fn, reps=20):
    for _ in range(3): fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def rule(K):
    p = H.GemmPlan()
    rc = H.lib().mca_dbg_plan_gemm_nt(H.PLAN_RES_LNBWD_TALL, C.byref(H.NtProblem(M=T, N=D, K=K)), cus, C.byref(p))
    return (160 if p.kernel == H.GK_NT_ROWS160_LNBWD else 128, p.nwg) if rc == 0 else (None, 0)


rows = {name: [] for name, _, _ in SHAPES}
for name, K, res in SHAPES:
    fn = launch(K, res)
    for p in range(pairs):
        t = {}
        for form in (("128", "160") if p % 2 == 0 else ("160", "128")):
            entry, knob = FORMS[form]
            dxa.normal_()          # (the in-place forms would otherwise feed their own output back 20 times)
            with H.knobs(**{f"k{H.KNOB_ROWS_HEIGHT}": knob}):
                t[form] = timed(lambda: fn(entry))
        rows[name].append(t)
        print(f"{name:16s} K={K:5d} pair {p}: 128 rows {t['128']:7.1f} us -> 160 rows {t['160']:7.1f} us ({t['160'] - t['128']:+6.1f})", flush=True)
print(f"T = {T}, D = {D}, {cus} CUs: {-(-T // 128)} tiles of 128 rows, {-(-T // 160)} of 160; us per launch")
for name, K, res in SHAPES:
    for form in ("128", "160"):
        v = sorted(r[form] for r in rows[name])
        print(f"{name:16s} K={K:5d} {form:3s} rows  min {v[0]:7.1f}  median {v[len(v) // 2]:7.1f}  max {v[-1]:7.1f}   (spread between pairs {v[-1] - v[0]:5.1f})")
    d = sorted(r["160"] - r["128"] for r in rows[name])
    h, nwg = rule(K)
    print(f"{name:16s} K={K:5d} 160 - 128: min {d[0]:+.1f}  median {d[len(d) // 2]:+.1f}  max {d[-1]:+.1f} us;  the rule picks {h} rows ({nwg} workgroups)")
