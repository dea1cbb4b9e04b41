"""FusionEngine.fuse_ln_rows at step level: the CMU configuration at depth 1, b = 2 (T = 5,076 token rows: 40 row tiles, the last one
partial), one forward + backward with the flag on and one with it off.  The fused launch (mca_gemm_nt_res_lnbwd) produces dx and
its bf16 copy bit for bit (tests/test_gemm_rows_gpu.py), so the loss, the pooled outputs and every gradient but the trunk norm
gammas are the same bits; the gammas - the only tensors the fused kernel adds into itself, with fp32 atomics - agree to the
atomic-order bound.

Two runs of ONE path have to be the same bits for that comparison to say anything, and by default they are not: kernels this
flag does not touch add parameter gradients with fp32 atomics (weight gradients split over rows, the row reductions, the encoder
norms).  Both runs therefore pin those orders through the measurement knobs - 3 = 1: one row split per weight gradient,
14 = 1: one workgroup for the LayerNorm backward kernels and mca_reduce_rows - and every modality is present (a dropped one's
mean(V) rows are atomic sums in the forward).  One sum no knob reaches: the affine pair of every encoder's input norm
(encoders.<name>.token_encoder.0.weight / .bias), which ln_bwd_params_kernel adds from up to 1,024 row slabs.  Those launches -
mca_layernorm_bwd asked for parameter gradients only, which the step does nowhere else - are sent through the fixed-order form
of the same entry (mca_layernorm_bwd_det) for the length of both runs, so these eight tensors are held bit for bit as well.
A second flag-off run is held to the first in the same way as the flag-on run, as the precondition."""
import copy
import importlib

import pytest
import torch

from util_small import rel_err

pytestmark = pytest.mark.gpu
B = 2
GAMMA_REL = 2 * 2e-5          # either sum is within 2e-5 of the exact one (tests/test_kernels_gpu.py, mca_layernorm_bwd's dgamma)
FUSED = "mca_gemm_nt_res_lnbwd"


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("mca-paper_amd")


class counting:
    """counts the calls of one entry point of the loaded library (hip.call looks the function up on the library object every time)"""

    def __init__(self, H, name):
        self.lib, self.name, self.n = H.lib(), name, 0

    def __enter__(self):
        self.fn = getattr(self.lib, self.name)

        def wrapped(*a):
            self.n += 1
            return self.fn(*a)
        setattr(self.lib, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.fn)


class ordered_param_norms:
    """sends every parameter-gradients-only call of mca_layernorm_bwd (no dx, no bf16 copy: an encoder's input norm) to
    mca_layernorm_bwd_det, which adds the row slabs' partial sums in ascending order; every other call goes through unchanged"""

    def __init__(self, H):
        self.lib, self.scratch, self.n = H.lib(), [], 0

    def __enter__(self):
        self.fn = self.lib.mca_layernorm_bwd

        def wrapped(*a):
            if a[10] is not None or a[12] is not None:          # dx / dx_bf16 wanted: a trunk or pooling norm
                return self.fn(*a)
            self.n += 1
            buf = torch.empty(max(1, self.lib.mca_layernorm_bwd_det_scratch(a[17], a[18])), device="cuda")
            self.scratch.append(buf)                             # alive until the run has been synchronised
            return self.lib.mca_layernorm_bwd_det(*a[:19], buf.data_ptr(), buf.numel(), a[19])
        self.lib.mca_layernorm_bwd = wrapped
        return self

    def __exit__(self, *exc):
        self.lib.mca_layernorm_bwd = self.fn


def run(P, cfg, batch, rows, deterministic=False):
    H = importlib.import_module("mca-paper_amd.hip")
    torch.manual_seed(43)
    model = P.MCA(**copy.deepcopy(cfg)).cuda()
    eng = model.engine
    eng.check_finite = False
    eng.fuse_ln_rows = rows
    if deterministic:
        eng.set_deterministic(True)
    H.profile_start({"mca_layernorm_bwd", "mca_gemm_nt"})
    try:
        with H.knobs(k3=1, k14=1), counting(H, FUSED) as fused, ordered_param_norms(H) as ordered:
            out = model(batch)
            out["loss"].backward()
            torch.cuda.synchronize()
        assert deterministic or ordered.n > 0          # (deterministic mode asks for the fixed-order form itself)
    finally:
        launched = H.profile_stop()
    ln_bwd = sum(v[0] for k, v in launched.items() if k.split("/")[0] in ("mca_layernorm_bwd", "mca_layernorm_bwd_det"))
    return dict(out={k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)},
                grads={n: p.grad.detach().clone() for n, p in model.named_parameters()}, fused=fused.n, ln_bwd=ln_bwd,
                rule=eng.ln_rows_backward(B * eng.N), T=B * eng.N)


@pytest.fixture(scope="module")
def steps(P):
    cfg = dict(P.config.cmu_model_config(batch_size=B), depth=1)
    batch = P.data.synthetic_batch(cfg, B, seed=1234, lengths="uniform", p_drop=0.0, device="cuda")
    return dict(on=run(P, cfg, batch, True), off=run(P, cfg, batch, False), off2=run(P, cfg, batch, False),
                det=run(P, cfg, batch, True, deterministic=True))


def is_gamma(name):
    """a trunk norm's gamma: the final norm's, or a layer's"""
    return name.endswith("norm.gamma")


def test_the_flag_routes_the_three_trunk_norms(steps):
    on, off, det = steps["on"], steps["off"], steps["det"]
    assert on["T"] == 5076 and on["rule"] and not off["rule"] and not det["rule"]
    assert on["fused"] == 3 and off["fused"] == 0          # both norms of the layer and the final norm
    assert off["ln_bwd"] - on["ln_bwd"] == 3
    assert det["fused"] == 0 and det["ln_bwd"] == off["ln_bwd"]          # deterministic mode keeps mca_layernorm_bwd_det


def test_two_flag_off_runs_are_the_same_bits(steps):
    off, off2 = steps["off"], steps["off2"]
    for k, v in off["out"].items():
        assert torch.equal(off2["out"][k], v), k
    differing = [n for n, g in off["grads"].items() if not is_gamma(n) and not torch.equal(off2["grads"][n], g)]
    assert not differing, differing
    worst = {n: rel_err(off2["grads"][n], g) for n, g in off["grads"].items() if is_gamma(n)}
    print(f"ln rows step: LayerNorm parameter gradients, flag off against flag off: {worst}")
    assert max(worst.values()) <= GAMMA_REL, worst


def test_loss_outputs_and_gradients_are_bit_identical(steps):
    on, off = steps["on"], steps["off"]
    assert set(on["out"]) == set(off["out"]) and "loss" in on["out"] and len(on["out"]) > 1
    for k, v in off["out"].items():
        assert torch.equal(on["out"][k], v), k
    names = [n for n in off["grads"] if not is_gamma(n)]
    assert len(names) >= 33 and len(off["grads"]) - len(names) <= 4           # every Linear, token, table and encoder norm gradient
    assert sum(".token_encoder.0." in n for n in names) == 8                  # ... the encoder input norms' weight and bias among them
    differing = {n: rel_err(on["grads"][n], off["grads"][n]) for n in names if not torch.equal(on["grads"][n], off["grads"][n])}
    print(f"ln rows step: {len(names)} gradients compared bit for bit, {len(differing)} differ: {differing}")
    assert not differing, differing
    assert all(bool(torch.isfinite(g).all()) for g in on["grads"].values()) and float(on["grads"]["layers.0.norm.gamma"].abs().max()) > 0


def test_gammas_agree_to_the_atomic_order_bound(steps):
    on, off = steps["on"], steps["off"]
    gammas = [n for n in off["grads"] if is_gamma(n)]
    assert {"norm.gamma", "layers.0.norm.gamma"} <= set(gammas), gammas          # the final norm and the layer's shared norm
    worst = {n: rel_err(on["grads"][n], off["grads"][n]) for n in gammas}
    print(f"ln rows step: LayerNorm parameter gradients, relative difference on against off: {worst}")
    for n, d in worst.items():
        assert d <= GAMMA_REL, (n, d)
