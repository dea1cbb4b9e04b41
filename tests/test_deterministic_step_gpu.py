"""Deterministic mode at step level (FusionEngine.set_deterministic, INTEGRATION.md "Deterministic mode"): loss, every gradient,
the gradient norm the clip coefficient is computed from, and every weight after FusedAdamW.step() are the same bits on every run -
eagerly, replayed from a hipGraph, and in a fresh process - and the default mode launches none of the deterministic forms."""
import copy
import importlib
import os
import subprocess
import sys

import pytest
import torch

from util_small import small_config, rel_err, to_device

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DET_ENTRY_POINTS = ("mca_gemm_tn_acc_det", "mca_gemm_tn_acc_group_det", "mca_layernorm_bwd_det", "mca_reduce_rows_det", "mca_tab_value_bwd_det")
PLAIN_ENTRY_POINTS = tuple(n[:-len("_det")] for n in DET_ENTRY_POINTS)


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("mca-paper_amd")


def full_config(P, kind, b):
    if kind == "tcga":
        return P.config.tcga_model_config(batch_size=b)
    cfg = P.config.cmu_model_config(batch_size=b, zorro=kind == "mma")
    cfg["depth"] = 1
    return cfg


def first_difference(model, a, b):
    """name of the first parameter whose slice of two flat buffers differs"""
    eng = model.engine
    for n, p in model.named_parameters():
        lo = eng.grad_of(p).data_ptr() - eng.gflat.data_ptr()
        sl = slice(lo // 4, lo // 4 + p.numel())
        if not torch.equal(a[sl], b[sl]):
            return n
    return None


def fwd_bwd(model, batch):
    for p in model.parameters():
        p.grad = None          # (a live flat view would make the backward accumulate)
    out = model(batch)
    out["loss"].backward()
    torch.cuda.synchronize()
    return out["loss"].detach().clone(), model.engine.gflat.clone()


# ------------------------------------------------------------------------------------------------ the full-size step
@pytest.mark.parametrize("kind,b", [("cmu", 32), ("mma", 32), ("tcga", 16)])
def test_full_size_step_is_bitwise_reproducible(P, kind, b):
    """Whole chip busy (the setting of test_attention_backward_bitwise_deterministic_at_cmu_size; the TCGA model for the tabular
    path): three forward + backward runs from the same weights give the same loss and the same bits in every gradient; the same
    step in default mode differs from it only as two default-mode steps differ from each other (tests/test_step_gpu.py: 8e-3
    rel-L2 per tensor, 2e-4 relative on the loss)."""
    cfg = full_config(P, kind, b)
    torch.manual_seed(43)
    model = P.MCA(**cfg).cuda()
    eng = model.engine
    eng.check_finite = False
    batch = P.data.synthetic_batch(cfg, b, seed=1234, lengths="uniform", p_drop=0.2, device="cuda")
    assert eng.deterministic is False
    fwd_bwd(model, batch)          # "from the same weights": a TabularEncoder's first forward renormalises its embedding rows in place (max_norm)
    l_def, g_def = fwd_bwd(model, batch)
    eng.set_deterministic(True)
    assert eng.deterministic is True
    runs = [fwd_bwd(model, batch) for _ in range(3)]
    assert bool(torch.isfinite(runs[0][1]).all()) and float(runs[0][1].abs().max()) > 0
    for l, g in runs[1:]:
        assert torch.equal(l, runs[0][0]), (float(l), float(runs[0][0]))
        assert torch.equal(g, runs[0][1]), f"first differing gradient: {first_difference(model, g, runs[0][1])}"
    l_det, g_det = runs[0]
    assert abs(float(l_det) - float(l_def)) <= 2e-4 * abs(float(l_def))
    for n, p in model.named_parameters():
        lo = (eng.grad_of(p).data_ptr() - eng.gflat.data_ptr()) // 4
        d = rel_err(g_det[lo:lo + p.numel()], g_def[lo:lo + p.numel()])
        assert d <= 8e-3, (n, d)


# ------------------------------------------------------------------------------------------------ training steps
def make(P, cfg, seed=43):
    optim = importlib.import_module("mca-paper_amd.optim")
    torch.manual_seed(seed)
    model = P.build_model(copy.deepcopy(cfg)).cuda()
    model.engine.check_finite = "deferred"
    model.engine.set_deterministic(True)
    return model, optim.FusedAdamW(model, lr=1e-3)


STEP_CASES = [("small-mca", 6), ("small-tab", 4), ("cmu", 8)]


def step_case(P, name, b):
    cfg = small_config(name[6:]) if name.startswith("small-") else full_config(P, name, b)
    if name.startswith("small-"):
        return cfg, to_device(P.data.synthetic_batch(cfg, b, seed=5, p_drop=0.3), "cuda")
    return cfg, P.data.synthetic_batch(cfg, b, seed=1234, lengths="uniform", p_drop=0.2, device="cuda")


@pytest.mark.parametrize("name,b", STEP_CASES)
def test_two_models_train_to_the_same_bits(P, name, b):
    """two models from the same seed, three FusedAdamW steps with clip 2.0 each: every weight, and the gradient norm of every step -
    the one word the clip coefficient is a function of (mca_adamw_step) - are bit-equal"""
    optim = importlib.import_module("mca-paper_amd.optim")
    cfg, batch = step_case(P, name, b)
    hist = []
    for _ in range(2):
        model, opt = make(P, cfg)
        norms = []
        for _s in range(3):
            out = model(batch); opt.zero_grad(); out["loss"].backward()
            norms.append(optim.clip_grad_norm_(model, 2.0).clone())
            opt.step()
        torch.cuda.synchronize()
        model.engine.assert_finite()
        hist.append((torch.stack(norms), model.engine.flat.clone(), model))
    (n0, w0, m0), (n1, w1, _) = hist
    assert torch.equal(n0, n1), (n0.tolist(), n1.tolist())
    assert torch.equal(w0, w1), f"first differing weight: {first_difference(m0, w0, w1)}"          # (flat and gflat share their layout)
    assert float(n0.min()) > 0


@pytest.mark.parametrize("name,b", [("small-mca", 6), ("cmu", 8)])
def test_graphed_step_in_deterministic_mode(P, name, b):
    """GraphedStep captures the mode the engine is in.  Two captured steps from the same state replay two steps to bit-equal weights
    and gradients; two eager runs of the same body are bit-equal; and eager equals replay - the same kernels in the same order on
    the same scratch, so the same bits are expected and asserted (profiles/deterministic_mode.md)."""
    graph = importlib.import_module("mca-paper_amd.graph")
    cfg, batch = step_case(P, name, b)
    res = {}
    for key, eager in (("replay-a", False), ("replay-b", False), ("eager-a", True), ("eager-b", True)):
        model, opt = make(P, cfg)
        g = graph.GraphedStep(model, opt, batch, clip=2.0)
        assert g.deterministic is True
        with pytest.raises(RuntimeError, match="set_deterministic"):
            model.engine.set_deterministic(False)          # a live captured step would go on replaying the other mode
        norms = []
        for _s in range(2):
            g.step(batch, eager=eager)
            norms.append(g.gnorm.clone())
        torch.cuda.synchronize()
        model.engine.assert_finite()
        res[key] = (torch.stack(norms), model.engine.flat.clone(), model.engine.gflat.clone(), model)
        del g
    for a, b_ in (("replay-a", "replay-b"), ("eager-a", "eager-b"), ("eager-a", "replay-a")):
        (na, wa, ga, m), (nb, wb, gb, _) = res[a], res[b_]
        assert torch.equal(ga, gb), f"{a} / {b_}: first differing gradient: {first_difference(m, ga, gb)}"
        assert torch.equal(na, nb) and torch.equal(wa, wb), f"{a} / {b_}: first differing weight: {first_difference(m, wa, wb)}"
    assert float(res["replay-a"][0].min()) > 0


# ------------------------------------------------------------------------------------------------ the switch
def test_mode_switch_and_default_mode_launches(P):
    hipm = importlib.import_module("mca-paper_amd.hip")
    graph = importlib.import_module("mca-paper_amd.graph")
    optim = importlib.import_module("mca-paper_amd.optim")
    cfg, batch = step_case(P, "small-tab", 4)
    torch.manual_seed(43)
    model = P.build_model(copy.deepcopy(cfg)).cuda()
    eng = model.engine
    assert eng.deterministic is False

    def launched():
        hipm.profile_start(DET_ENTRY_POINTS + PLAIN_ENTRY_POINTS)
        try:
            fwd_bwd(model, batch)
        finally:
            tot = hipm.profile_stop()
        return {k.split("/")[0] for k, (n, _, _) in tot.items() if n > 0}
    got = launched()
    assert got and got <= set(PLAIN_ENTRY_POINTS), got          # mode off: none of the deterministic forms is launched
    eng.set_deterministic(True)
    got = launched()
    assert got and got <= set(DET_ENTRY_POINTS), got            # mode on: none of the atomic forms
    assert {"mca_layernorm_bwd_det", "mca_reduce_rows_det", "mca_tab_value_bwd_det", "mca_gemm_tn_acc_det"} <= got
    eng.set_deterministic(False)
    assert eng.deterministic is False
    # a live captured step pins the mode
    opt = optim.FusedAdamW(model, lr=1e-3)
    g = graph.GraphedStep(model, opt, batch, clip=2.0)
    assert g.deterministic is False
    eng.set_deterministic(False)          # no change: fine
    with pytest.raises(RuntimeError, match="set_deterministic"):
        eng.set_deterministic(True)
    del g
    eng.set_deterministic(True)
    assert eng.deterministic is True


def test_debug_switch_in_a_fresh_process(P):
    code = ("import importlib, sys, torch; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests');"
            "P = importlib.import_module('mca-paper_amd'); from util_small import small_config;"
            "m = P.MCA(**small_config('mca')).cuda(); print('deterministic', m.engine.deterministic)")
    r = subprocess.run([sys.executable, "-c", code, REPO], env=dict(os.environ, MCA_DEBUG="deterministic=1"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "deterministic True" in r.stdout, r.stdout[-2000:]
