"""FusionEngine.qkv_head_major at step level: the CMU configuration at depth 1, b = 8 (T = 20,304 token rows; the layer attention's
backward is the one-pass kernel, key blocks split 4 ways), one forward + backward with q | k | v and dO head-major from their GEMMs
(the default there) and one with MCA_DEBUG=qkv_hm=0.  Every kernel reads the same values in the same order in both layouts
(tests/test_gemm_cb_gpu.py, tests/test_attention_hm_gpu.py), so the loss, the pooled tokens and dq | dk | dv are the same bits, and in
deterministic mode - every parameter gradient summed in a fixed order - so is every gradient.  30 % of the modalities are dropped:
uniform rows, mean(V) and dvmean take part.

Where the head-major form does not apply the engine keeps the row-major one without a word - a forward that is read out
afterwards (attention_readout), fp8 operands, knob 7 = 1 (no 256 x 256 persistent GEMM) - and still computes what the flag-off run
computes.  The captured step (graph.GraphedStep) replays with the layout it was captured with."""
import copy
import importlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
B = 8
RECORDED = ("mca_attn_fwd", "mca_attn_fwd_fp8", "mca_attn_quant_mxfp8", "mca_attn_bwd_prep", "mca_attn_bwd_prep_onepass", "mca_attn_bwd_onepass",
            "mca_attn_bwd_dq", "mca_attn_bwd_dkv", "mca_attn_quant_bwd_mxfp8", "mca_attn_bwd_dq_fp8", "mca_attn_bwd_dkv_fp8", "mca_gemm_nt",
            "mca_attn_vmean_if_needed", "mca_attn_vmean")


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("mca-paper_amd")


@pytest.fixture(scope="module")
def setup(P):
    cfg = dict(P.config.cmu_model_config(batch_size=B), depth=1)
    batch = P.data.synthetic_batch(cfg, B, seed=1234, lengths="uniform", p_drop=0.3, device="cuda")
    return cfg, batch


def build(P, cfg, flag, deterministic=False, fp8=False):
    """a freshly seeded model whose engine read MCA_DEBUG=qkv_hm=0 (flag off) or nothing (flag on) at construction"""
    old = os.environ.get("MCA_DEBUG")
    if not flag:
        os.environ["MCA_DEBUG"] = "qkv_hm=0"
    else:
        os.environ.pop("MCA_DEBUG", None)
    try:
        torch.manual_seed(43)
        model = P.MCA(**copy.deepcopy(cfg)).cuda()
        eng = model.engine          # (built on first access: that is when MCA_DEBUG is read)
    finally:
        os.environ.pop("MCA_DEBUG", None)
        if old is not None:
            os.environ["MCA_DEBUG"] = old
    assert eng.dbg["qkv_hm"] == flag
    eng.check_finite = False
    if deterministic:
        eng.set_deterministic(True)
    if fp8:
        eng.set_attention_dtype("fp8")
    return model


def run(P, cfg, batch, flag, knobs=None, **kw):
    H = importlib.import_module("mca-paper_amd.hip")
    model = build(P, cfg, flag, **kw)
    eng = model.engine
    H.profile_start(RECORDED)
    try:
        with H.knobs(**(knobs or {})):
            out = model(batch)
            out["loss"].backward()
            torch.cuda.synchronize()
    finally:
        launched = H.profile_stop()
    ws = eng.workspace(B)
    a = ws["layers"][0]
    return dict(loss=out["loss"].detach().clone(), pooled=ws["pooled"].clone(), dqkv=a["dqkv"].clone(), lse=a["lse"].clone(), o=a["o"].clone(),
                grads={n: p.grad.detach().clone() for n, p in model.named_parameters()}, launched={k: v[0] for k, v in launched.items()},
                qkv_hm=a["qkv_hm"], do_hm=ws["do_hm"], form=eng.backward_plan(ws, B, eng.N), packed="q_hm" in ws)


@pytest.fixture(scope="module")
def steps(P, setup):
    cfg, batch = setup
    return dict(on=run(P, cfg, batch, True, deterministic=True), off=run(P, cfg, batch, False, deterministic=True))


def test_the_flag_routes_the_layout(steps):
    on, off = steps["on"], steps["off"]
    assert tuple(on["form"]) == tuple(off["form"]) == ("onepass", 4)
    assert on["qkv_hm"] is True and on["do_hm"] is True and not on["packed"]          # no packed copies were ever allocated
    assert off["qkv_hm"] is False and off["do_hm"] is False and off["packed"]


def test_loss_pooled_and_attention_gradients_are_bit_identical(steps):
    on, off = steps["on"], steps["off"]
    assert bool(torch.isfinite(on["loss"])) and bool(torch.isinf(on["lse"]).any())          # uniform rows exist: vmean and dvmean take part
    for k in ("loss", "pooled", "o", "lse", "dqkv"):
        assert torch.equal(on[k], off[k]), k
    assert float(on["dqkv"].float().abs().max()) > 0


def test_every_parameter_gradient_is_bit_identical_in_deterministic_mode(steps):
    on, off = steps["on"], steps["off"]
    assert set(on["grads"]) == set(off["grads"]) and len(on["grads"]) >= 33
    differing = [n for n, g in off["grads"].items() if not torch.equal(on["grads"][n], g)]
    assert not differing, differing
    assert all(bool(torch.isfinite(g).all()) for g in on["grads"].values())
    assert float(on["grads"]["layers.0.attn.to_q.weight"].abs().max()) > 0 and float(on["grads"]["layers.0.attn.to_kv.weight"].abs().max()) > 0


def test_the_recorded_launches_are_unchanged(steps):
    """the new entry points are timed in the rows of the ones they replace: same keys (GEMM shape tags included), same counts"""
    on, off = steps["on"], steps["off"]
    assert on["launched"] == off["launched"], (on["launched"], off["launched"])
    assert on["launched"]["mca_attn_bwd_prep_onepass"] == 1 and on["launched"]["mca_attn_bwd_onepass/layer"] == 1
    assert on["launched"]["mca_attn_fwd/layer"] == 1 and on["launched"]["mca_attn_vmean_if_needed"] == 2          # the layer's and the pooling's
    T = B * 2538
    assert on["launched"][f"mca_gemm_nt/{T}x1536x512"] == 1 and on["launched"][f"mca_gemm_nt/{T}x512x512"] >= 1


@pytest.mark.parametrize("what", ["fp8", "knob7"])
def test_fallbacks_keep_the_row_major_layout_and_match_the_flag_off_run(P, setup, what):
    cfg, batch = setup
    kw = dict(fp8=True, deterministic=True) if what == "fp8" else dict(knobs=dict(k7=1), deterministic=True)
    on, off = run(P, cfg, batch, True, **kw), run(P, cfg, batch, False, **kw)
    assert on["qkv_hm"] is False and on["do_hm"] is False and on["form"].form == "onepass"
    assert on["launched"] == off["launched"]
    for k in ("loss", "pooled", "o", "lse", "dqkv"):          # (the forward and the attention backward have no order-dependent sum)
        assert torch.equal(on[k], off[k]), (what, k)


def test_a_forward_that_is_read_out_keeps_the_row_major_layout(P, setup):
    cfg, batch = setup
    res = {}
    for flag in (True, False):
        model = build(P, cfg, flag)
        model.eval()
        res[flag] = model.attention_readout(batch, probs_rows={0: (5, 3)})
        a = model.engine.workspace(B)["layers"][0]
        assert a["qkv_hm"] is False and not model.engine.rows_only
        if flag:          # the next training forward of the same engine is head-major again
            model.train()
            model(batch)
            assert a["qkv_hm"] is True
    assert torch.equal(res[True]["layer_mass"][0], res[False]["layer_mass"][0]) and torch.equal(res[True]["probs"][0], res[False]["probs"][0])
    assert torch.equal(res[True]["pool_mass"], res[False]["pool_mass"])


def test_captured_step_replays_with_the_head_major_layout(P, setup):
    """two replays and one eager step, each from the same weights, moments and step count: the forward has no order-dependent sum, so
    the three losses are the same number"""
    cfg, batch = setup
    optim = importlib.import_module("mca-paper_amd.optim")
    graph = importlib.import_module("mca-paper_amd.graph")
    model = build(P, cfg, True)
    eng = model.engine
    eng.check_finite = "deferred"
    opt = optim.FusedAdamW(model, lr=1e-5)
    g = graph.GraphedStep(model, opt, batch, clip=2.0)
    state = (eng.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count)
    a = eng.workspace(B)["layers"][0]
    losses = []
    for eager in (False, False, True):
        eng.flat.copy_(state[0]); opt.exp_avg.copy_(state[1]); opt.exp_avg_sq.copy_(state[2]); opt.step_count = state[3]
        eng.invalidate_weights()
        loss = g.step(batch, eager=eager)
        torch.cuda.synchronize()
        losses.append(float(loss))
        assert a["qkv_hm"] is True and eng.workspace(B)["do_hm"] is True
        assert bool(torch.isfinite(eng.gflat).all()) and not torch.equal(eng.flat, state[0])          # the step trained
    assert losses[0] == losses[1] == losses[2] and losses[0] == losses[0], losses
    eng.assert_finite()
