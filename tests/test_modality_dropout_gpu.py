"""GPU tests of the per-step modality dropout: mca_pack_masks_drop / mca_counter_add element by element against the CPU restatement
(tests/modality_dropout_util.py), the training step against its host-masked twin, the device step counter in eager and replayed
steps, and the engine's argument errors."""
import copy
import ctypes as C
import importlib
import itertools
import math

import numpy as np
import pytest
import torch

import modality_dropout_util as U
from util_small import small_config, rel_err, to_device

pytestmark = pytest.mark.gpu

BADARG, ALIGN = -1, -2          # MCA_E_BADARG, MCA_E_ALIGN (include/mca_hip.h)
DIMS = [1, 63, 64, 257, 300]    # below, at and across the wavefront (64) and the workgroup's 256-thread stride
RATES = [0.0, 1.0, 0.25, 0.5, 0.5]
EDGE_RAW = [[1, 1, 1, 1, 1], [0, 1, 0, 0, 0], [0, 1, 0, 1, 1], [0, 1, 1, 0, 0], [0, 0, 0, 0, 0]]          # edge_masks: sample x modality


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("mca-paper_amd")


# ------------------------------------------------------------------------------------------------ kernel level
def pack_args(H, masks, dims, n_tokens, n_fusion, rowm):
    pk = H.PackMasksArgs()
    off, offsets = 0, []
    for i, (mk, n) in enumerate(zip(masks, dims)):
        d = pk.m[i]
        d.mask, d.elem_bytes, d.n, d.offset = mk.data_ptr(), mk.element_size(), n, off
        d.rowmask = rowm[i].data_ptr() if rowm is not None else None
        offsets.append(off)
        off += n
    pk.n_mod, pk.batch, pk.n_tokens, pk.n_fusion = len(dims), masks[0].shape[0], n_tokens, n_fusion
    return pk, offsets


def drop_args(H, p, seed, sample0, keep_one):
    da = H.ModalityDropArgs()
    for i, v in enumerate(p):
        da.p[i] = v
    da.seed, da.sample0, da.keep_one = seed, sample0, int(keep_one)
    return da


def run_drop(H, masks, dims, gap, F, with_rowmasks, p, seed, step, sample0, keep_one, with_dropped=True):
    """one launch on sentinel-filled outputs -> (padding, rowmasks or None, present, dropped or None, offsets, n_tokens)"""
    b = masks[0].shape[0]
    N = sum(dims) + gap + F
    rowm = [torch.full((b * n,), 9, device="cuda", dtype=torch.uint8) for n in dims] if with_rowmasks else None
    pk, offsets = pack_args(H, masks, dims, N, F, rowm)
    padding = torch.full((b, N), 255, device="cuda", dtype=torch.uint8)
    present = torch.full((b,), -1, device="cuda", dtype=torch.int32)
    dropped = torch.full((b,), -1, device="cuda", dtype=torch.int32) if with_dropped else None
    t = torch.tensor([step], device="cuda", dtype=torch.int64)
    da = drop_args(H, p, seed, sample0, keep_one)
    H.call("mca_pack_masks_drop", C.byref(pk), C.byref(da), t.data_ptr(), padding.data_ptr(), present.data_ptr(),
           dropped.data_ptr() if with_dropped else None, H.stream_ptr())
    torch.cuda.synchronize()
    assert int(t[0]) == step          # the counter is only read
    return padding, rowm, present, dropped, offsets, N


def edge_masks(elem_bytes, b=5):
    """b = 5 samples over DIMS, raw presence EDGE_RAW: sample 0 has every modality; sample 1 only the p = 1 modality, so keep_one
    must rescue it at every draw; sample 2 lacks the p = 0 modality and one more; sample 3 lacks the p = 0 modality and has its two
    0.5-rate modalities fully padded already; sample 4 has nothing at all.  Samples 1-3 can lose everything they have although the
    absent p = 0 modality is never wanted, and their rescue is the argmax of u over a strict subset of the modalities."""
    g = torch.Generator().manual_seed(12)
    masks = [torch.rand(b, n, generator=g) < 0.4 for n in DIMS]
    for i, m in enumerate(masks):
        for s in range(b):
            if EDGE_RAW[s][i]:
                m[s, 0] = False          # (keeps a valid token whatever the random mask says; n = 1: its one token)
            else:
                m[s] = True
    if elem_bytes == 8:
        return [(m.to(torch.int64) * 7).cuda() for m in masks]          # any non-zero value = padded
    return [m.to(torch.uint8).cuda() for m in masks]


@pytest.mark.parametrize("keep_one", [False, True])
@pytest.mark.parametrize("elem_bytes", [1, 8])
def test_kernel_matches_restatement(H, elem_bytes, keep_one):
    """padding, every row mask, presence bits and drop bits, exactly, over n_fusion 0 / 8, row masks given / NULL, sample0 0 / 1000,
    step 0 / 2^33 + 5 and two seeds; the gap the descriptors leave in a row keeps its sentinel and the inputs keep their bits.
    With keep_one the restated draws rescue in samples that lack modalities (edge_masks): the test asserts that of its own
    restatement, so the rescue condition over the raw-present modalities only, and their argmax, are what the kernel is held to."""
    masks = edge_masks(elem_bytes)
    before = [m.clone() for m in masks]
    host = [m.cpu().numpy() for m in masks]
    rescued_total = among_several = absent_is_larger = not_the_sure_one = 0
    for F, with_rm, sample0, step, seed in itertools.product((0, 8), (True, False), (0, 1000), (0, 2 ** 33 + 5), (42, 0xDEADBEEFCAFEF00D)):
        padding, rowm, present, dropped, offsets, N = run_drop(H, masks, DIMS, 3, F, with_rm, RATES, seed, step, sample0, keep_one)
        e = U.expected(host, offsets, N, F, RATES, seed, step, sample0, keep_one)
        case = (F, with_rm, sample0, step, hex(seed))
        assert np.array_equal(padding.cpu().numpy(), e["padding"]), case
        assert np.array_equal(present.cpu().numpy(), e["present"]), case
        assert np.array_equal(dropped.cpu().numpy(), e["dropped"]), case
        if with_rm:
            for i, r in enumerate(rowm):
                assert np.array_equal(r.cpu().numpy(), e["rowmasks"][i]), (case, i)
        # what the rates pin whatever the draw: p = 0 never; p = 1 always unless rescued, and its bit is set in the empty sample too
        assert not (e["dropped"] & 1).any() and e["present"][4] == 0 and (e["dropped"][4] >> 1) & 1
        assert keep_one or ((e["dropped"] >> 1) & 1).all()
        assert e["rescued"][4] == -1 and (not keep_one or (e["present"][:4] != 0).all())
        assert np.array_equal(e["raw"], np.array(EDGE_RAW, dtype=bool))
        rescued_total += int((e["rescued"] >= 0).sum())
        if keep_one:
            assert e["rescued"][1] == 1 and e["present"][1] == 2          # its only modality has p = 1: rescued at every draw
        for s in np.nonzero(e["rescued"] >= 0)[0]:
            r, raw, u = e["rescued"][s], e["raw"][s], e["u"][s]
            assert raw[r] and not raw.all() and u[r] == u[raw].max()
            among_several += int(raw.sum() >= 2)
            absent_is_larger += int((u[~raw] > u[r]).any())          # an argmax over ALL modalities would have picked an absent one
            not_the_sure_one += int(r != 1)
    for m, m0 in zip(masks, before):
        assert torch.equal(m, m0)
    if not keep_one:
        assert rescued_total == 0
    else:
        # the draws this case stands on (each distinct draw is launched four times: n_fusion x row masks): rescues happen, some
        # among two or more raw-present modalities, some with a larger u on an absent modality, some of another than the p = 1 one
        print(f"keep_one: {rescued_total} rescues, {among_several} among >= 2 present, {absent_is_larger} with a larger absent u, "
              f"{not_the_sure_one} of another modality than the p = 1 one")
        assert rescued_total >= 32 and among_several > 0 and absent_is_larger > 0 and not_the_sure_one > 0


def test_dropped_may_be_null(H):
    masks = edge_masks(1)
    host = [m.cpu().numpy() for m in masks]
    padding, rowm, present, _, offsets, N = run_drop(H, masks, DIMS, 0, 8, True, RATES, 42, 1, 0, True, with_dropped=False)
    e = U.expected(host, offsets, N, 8, RATES, 42, 1, 0, True)
    assert np.array_equal(padding.cpu().numpy(), e["padding"]) and np.array_equal(present.cpu().numpy(), e["present"])


@pytest.mark.parametrize("elem_bytes", [1, 8])
def test_all_rates_zero_equals_pack_masks(H, elem_bytes):
    masks = edge_masks(elem_bytes)
    b, F = 5, 8
    padding, rowm, present, dropped, offsets, N = run_drop(H, masks, DIMS, 3, F, True, [0.0] * 5, 42, 7, 0, True)
    rowm2 = [torch.full((b * n,), 9, device="cuda", dtype=torch.uint8) for n in DIMS]
    pk, _ = pack_args(H, masks, DIMS, N, F, rowm2)
    padding2 = torch.full((b, N), 255, device="cuda", dtype=torch.uint8)
    present2 = torch.full((b,), -1, device="cuda", dtype=torch.int32)
    H.call("mca_pack_masks", C.byref(pk), padding2.data_ptr(), present2.data_ptr(), H.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(padding, padding2) and torch.equal(present, present2) and int(dropped.abs().max()) == 0
    for a, c in zip(rowm, rowm2):
        assert torch.equal(a, c)


def test_sample0_halves_give_the_rows_of_one_launch(H):
    g = torch.Generator().manual_seed(3)
    dims, p = [5, 70, 300], [0.5, 0.5, 0.5]
    masks = [(torch.rand(8, n, generator=g) < 0.3).to(torch.uint8).cuda() for n in dims]
    full = run_drop(H, masks, dims, 0, 8, True, p, 42, 2, 0, True)
    for lo in (0, 4):
        half = run_drop(H, [m[lo:lo + 4].contiguous() for m in masks], dims, 0, 8, True, p, 42, 2, lo, True)
        assert torch.equal(half[0], full[0][lo:lo + 4]) and torch.equal(half[2], full[2][lo:lo + 4]) and torch.equal(half[3], full[3][lo:lo + 4])
        for i, n in enumerate(dims):
            assert torch.equal(half[1][i], full[1][i][lo * n:(lo + 4) * n])
    assert int(full[3].max()) > 0 and not torch.equal(full[3][:4], full[3][4:])


def test_argument_checks(H):
    """every refusal launches nothing: the sentinels stay"""
    masks = edge_masks(1)
    pk, _ = pack_args(H, masks, DIMS, sum(DIMS) + 8, 8, None)
    padding = torch.full((5, sum(DIMS) + 8), 255, device="cuda", dtype=torch.uint8)
    present = torch.full((5,), -1, device="cuda", dtype=torch.int32)
    dropped = torch.full((5,), -1, device="cuda", dtype=torch.int32)
    t = torch.zeros(2, device="cuda", dtype=torch.int64)
    f, s = H.lib().mca_pack_masks_drop, H.stream_ptr()
    ok = drop_args(H, RATES, 42, 0, True)
    out = (padding.data_ptr(), present.data_ptr(), dropped.data_ptr())
    assert f(C.byref(pk), None, t.data_ptr(), *out, s) == BADARG
    assert f(C.byref(pk), C.byref(ok), None, *out, s) == BADARG
    for i, v in [(2, float("nan")), (0, -0.1), (4, 1.5), (15, 2.0), (3, float("inf"))]:
        bad = drop_args(H, RATES, 42, 0, True)
        bad.p[i] = v
        assert f(C.byref(pk), C.byref(bad), t.data_ptr(), *out, s) == BADARG, (i, v)
    assert f(C.byref(pk), C.byref(ok), t.data_ptr() + 4, *out, s) == ALIGN
    # mca_pack_masks' own checks still hold
    assert f(None, C.byref(ok), t.data_ptr(), *out, s) == BADARG
    assert f(C.byref(pk), C.byref(ok), t.data_ptr(), None, out[1], out[2], s) == BADARG
    assert f(C.byref(pk), C.byref(ok), t.data_ptr(), out[0], None, out[2], s) == BADARG
    pk.n_tokens = sum(DIMS) + 7
    assert f(C.byref(pk), C.byref(ok), t.data_ptr(), *out, s) == BADARG
    add = H.lib().mca_counter_add
    assert add(None, 1, s) == BADARG and add(t.data_ptr() + 4, 1, s) == ALIGN
    torch.cuda.synchronize()
    assert int(padding.min()) == 255 and int(present.max()) == -1 and int(dropped.max()) == -1 and t.tolist() == [0, 0]


def test_counter_add(H):
    t = torch.tensor([2 ** 33 + 5, 77], device="cuda", dtype=torch.int64)
    H.call("mca_counter_add", t.data_ptr(), 1, H.stream_ptr())
    H.call("mca_counter_add", t.data_ptr(), 5, H.stream_ptr())
    torch.cuda.synchronize()
    assert t.tolist() == [2 ** 33 + 11, 77]


def test_statistics_on_the_device(H):
    """4096 samples x 4 one-token modalities at p = 0.5: the device's draw is the restatement's, and that is within 4 sigma"""
    b, M, p = 4096, 4, 0.5
    masks = [torch.zeros(b, 1, device="cuda", dtype=torch.uint8) for _ in range(M)]
    _, _, present, dropped, _, _ = run_drop(H, masks, [1] * M, 0, 0, False, [p] * M, 42, 0, 0, False)
    want, _, _ = U.draw(np.ones((b, M), dtype=bool), [p] * M, 42, 0, keep_one=False)
    got = ((dropped.cpu().numpy()[:, None] >> np.arange(M)[None, :]) & 1).astype(bool)
    assert np.array_equal(got, want) and np.array_equal(present.cpu().numpy(), 15 - dropped.cpu().numpy())
    z_all = abs(want.mean() - p) / math.sqrt(p * (1 - p) / (b * M))
    z_mod = np.abs(want.mean(0) - p) / math.sqrt(p * (1 - p) / b)
    print(f"device draw: overall {z_all:.2f} sigma, per modality {np.round(z_mod, 2).tolist()}")
    assert z_all <= 4.0 and (z_mod <= 4.0).all()


# ------------------------------------------------------------------------------------------------ step level
B, SEED = 8, 42


def full_batch(P, cfg, seed=5):
    """every modality present in every sample: the draw alone decides what goes"""
    return to_device(P.data.synthetic_batch(cfg, B, seed=seed, p_drop=0.0), "cuda")


def restated(cfg, step, b=B, p=0.5, keep_one=True):
    M = len(cfg["encoder_configs"])
    return U.draw(np.ones((b, M), dtype=bool), [p] * M, SEED, step, keep_one=keep_one)


def build(P, cfg, deterministic=True, lr=1e-3):
    optim = importlib.import_module("mca-paper_amd.optim")
    torch.manual_seed(43)
    model = P.build_model(copy.deepcopy(cfg)).cuda()
    model.engine.check_finite = "deferred"
    model.engine.set_deterministic(deterministic)
    return model, optim.FusedAdamW(model, lr=lr)


def all_half(model):
    return {n: 0.5 for n in model.modality_types}


@pytest.mark.parametrize("variant", ["mca", "tab", "eao"])
def test_step_equals_its_host_masked_twin(P, variant):
    """on-device dropout against the step without it on a copy of the batch whose attention masks carry the restated drop matrix
    (data untouched): loss, pooled outputs, sample masks and, in deterministic mode, every gradient, bit for bit"""
    cfg = small_config(variant)
    names = list(cfg["encoder_configs"])
    batch = full_batch(P, cfg)
    want, rescued, _ = restated(cfg, 0)
    # the draw this test stands on: one rescued sample, two kept whole (a draw that keeps everything would pass silently)
    assert int((rescued >= 0).sum()) == 1 and int((~want).all(1).sum()) == 2 and want.any()
    twin = copy.deepcopy(batch)
    for i, n in enumerate(names):
        am = twin[n]["attention_mask"]
        row = torch.from_numpy(want[:, i]).to(am.device)[:, None]
        twin[n]["attention_mask"] = (am.bool() | row).to(am.dtype)
    res = []
    for drop, bt in ((True, batch), (False, twin)):
        model, _ = build(P, cfg)
        if drop:
            model.engine.set_modality_dropout(all_half(model), seed=SEED, keep_one=True, step=0)
        out = model(bt)
        model.zero_grad()
        out["loss"].backward()
        torch.cuda.synchronize()
        model.engine.assert_finite()
        res.append((out, {n: p.grad.detach().clone() for n, p in model.named_parameters()}, model))
    (od, gd, md), (ot, gt, _) = res
    assert "modality_dropped" in od and "modality_dropped" not in ot
    assert np.array_equal(od["modality_dropped"].cpu().numpy(), want)
    assert md.engine.modality_dropout_step() == 1
    assert torch.equal(od["loss"], ot["loss"]), (float(od["loss"]), float(ot["loss"]))
    for k in md.output_slots():
        assert torch.equal(od[k], ot[k]), k
    for i, n in enumerate(names):
        assert torch.equal(od["modality_sample_mask"][n], ot["modality_sample_mask"][n]), n
        assert np.array_equal(od["modality_sample_mask"][n].cpu().numpy(), ~want[:, i]), n
    for k in od["losses"]:
        assert torch.equal(od["losses"][k], ot["losses"][k]) or (bool(torch.isnan(od["losses"][k])) and bool(torch.isnan(ot["losses"][k]))), k
    for n in gt:
        assert torch.equal(gd[n], gt[n]), n
    assert max(float(g.abs().max()) for g in gd.values()) > 0


def test_counter_and_launches(P):
    """training forwards draw t, t + 1; eval() and no_loss forwards in between neither drop nor move the counter; with the feature
    off the launches of a step are those of an engine that never heard of it"""
    hipmod = importlib.import_module("mca-paper_amd.hip")
    mods = [hipmod] + [importlib.import_module("mca-paper_amd." + m) for m in ("encoder_steps", "engine")]
    cfg = small_config("mca")
    batch = full_batch(P, cfg)
    model, _ = build(P, cfg, deterministic=False)
    eng = model.engine

    def launches():
        seen, real = [], hipmod.call

        def recording(name, *a, **k):
            seen.append(name)
            return real(name, *a, **k)
        try:
            for m in mods:
                m.call = recording
            out = model(batch)
        finally:
            for m in mods:
                m.call = real
        return seen, out

    assert eng.modality_dropout is None and eng.modality_dropout_step() == 0
    model(batch)          # (the first forward also builds the bf16 weight copies)
    never, _ = launches()
    assert "mca_pack_masks" in never and not {"mca_pack_masks_drop", "mca_counter_add"} & set(never)
    t = 2 ** 33 + 5
    eng.set_modality_dropout(all_half(model), seed=SEED, keep_one=True, step=t)
    assert eng.modality_dropout == {"rates": all_half(model), "seed": SEED, "keep_one": True} and eng.modality_dropout_step() == t
    on, out0 = launches()
    i = on.index("mca_pack_masks_drop")
    assert on[i + 1] == "mca_counter_add" and "mca_pack_masks" not in on and on[:i] + ["mca_pack_masks"] + on[i + 2:] == never
    assert np.array_equal(out0["modality_dropped"].cpu().numpy(), restated(cfg, t)[0])
    assert eng.modality_dropout_step() == t + 1
    model.eval()
    quiet, out_eval = launches()
    model.train()
    with torch.no_grad():
        out_nl = model(batch, no_loss=True)
    for o in (out_eval, out_nl):
        assert "modality_dropped" not in o and all(bool(v.all()) for v in o["modality_sample_mask"].values())
    assert quiet == never and eng.modality_dropout_step() == t + 1
    out1 = model(batch)
    assert np.array_equal(out1["modality_dropped"].cpu().numpy(), restated(cfg, t + 1)[0])
    assert not np.array_equal(restated(cfg, t)[0], restated(cfg, t + 1)[0]) and eng.modality_dropout_step() == t + 2
    # off again (all rates zero): today's launches, and the step restarts where it is told to
    eng.set_modality_dropout({n: 0.0 for n in model.modality_types}, step=3)
    assert eng.modality_dropout is None and eng.modality_dropout_step() == 3
    off, out_off = launches()
    assert off == never and "modality_dropped" not in out_off and eng.modality_dropout_step() == 3
    eng.set_modality_dropout(None)
    assert eng.modality_dropout is None


def test_graphed_step_draws_a_new_mask_at_every_replay(P):
    """constructing a GraphedStep leaves the counter alone; three replays give the masks of t, t + 1, t + 2 with no host work and
    end at t + 3; loss and weights follow three eager steps from the same state within the bound of
    tests/test_graph_gpu.py::test_graphed_step_matches_eager (3 x the eager loop's drift against itself + 2e-3 on the loss,
    + 1e-3 rel-L2 on the weights)"""
    optim = importlib.import_module("mca-paper_amd.optim")
    graph = importlib.import_module("mca-paper_amd.graph")
    cfg = small_config("mca")
    names = list(cfg["encoder_configs"])
    batch = full_batch(P, cfg)
    t0, runs = 3, []
    for graphed in (False, False, True):
        model, opt = build(P, cfg, deterministic=False)
        eng = model.engine
        eng.set_modality_dropout(all_half(model), seed=SEED, keep_one=True, step=t0)
        losses, snaps = [], []
        if graphed:
            g = graph.GraphedStep(model, opt, batch, clip=2.0, warmup=2)
            assert eng.modality_dropout_step() == t0 and opt.step_count == 0
            with pytest.raises(RuntimeError, match="set_modality_dropout"):
                eng.set_modality_dropout(None)
            with pytest.raises(RuntimeError, match="set_modality_dropout"):
                eng.set_modality_dropout(all_half(model), step=0)
        for i in range(3):
            if graphed:
                losses.append(float(g.step(batch)))
                out = g.out
            else:
                out = model(batch); opt.zero_grad(); out["loss"].backward(); optim.clip_grad_norm_(model, 2.0); opt.step()
                losses.append(float(out["loss"].detach()))
            torch.cuda.synchronize()
            want = restated(cfg, t0 + i)[0]
            assert np.array_equal(out["modality_dropped"].cpu().numpy(), want), (graphed, i)
            for k, n in enumerate(names):
                assert np.array_equal(out["modality_sample_mask"][n].cpu().numpy(), ~want[:, k]), (graphed, i, n)
            snaps.append(eng.flat.clone())
        assert eng.modality_dropout_step() == t0 + 3
        eng.assert_finite()
        runs.append((losses, snaps))
    (le, se), (le2, se2), (lg, sg) = runs
    drift_l = [abs(a - c) / abs(a) for a, c in zip(le, le2)]
    drift_w = [rel_err(a, c) for a, c in zip(se, se2)]
    print("eager-eager loss drift", drift_l, "weights", drift_w)
    print("graph-eager loss drift", [abs(a - c) / abs(a) for a, c in zip(le, lg)], "weights", [rel_err(a, c) for a, c in zip(se, sg)])
    for i in range(3):
        assert abs(le[i] - lg[i]) <= 3 * drift_l[i] * abs(le[i]) + 2e-3 * abs(le[i]), (i, le, le2, lg)
        assert rel_err(sg[i], se[i]) <= 3 * drift_w[i] + 1e-3, (i, rel_err(sg[i], se[i]), drift_w[i])
    assert len({restated(cfg, t0 + i)[0].tobytes() for i in range(3)}) == 3          # three different masks were asked for


def test_train_script_draws_from_the_yaml(P, tmp_path):
    """train_accel_gpu.py with `batch_dropout: true`, replayed loop: the logged batch_dropout_rate of step k is the mean of the
    restated drop matrix of t = k - 1 (seed: the YAML's `seed`, rates: modality_config[name]["dropout"]), so the script switched
    the feature on before the capture and every replay drew a new mask"""
    import json, os, subprocess, sys, yaml
    from conftest import REPO
    cfg = small_config("mca")
    rates = {"audio": 0.5, "video": 0.25, "text": 0.75}
    mod_cfg = {name: {"type": "embedded_sequence", "pad_len": enc["max_tokens"], "embedding_size": enc["input_size"], "data_col_name": "data",
                      "dropout": rates[name]} for name, enc in cfg["encoder_configs"].items()}
    out = tmp_path / "out"
    y = dict(encoder_configs=cfg["encoder_configs"], modality_config=mod_cfg, hidden_size=cfg["dim"], layers=cfg["depth"], heads=cfg["heads"],
             dim_head=cfg["dim_head"], num_fusion_tokens=cfg["num_fusion_tokens"], batch_size=4, fcl=cfg["fcl"], fcl_root=cfg["fcl_root"],
             bimodal_contrastive=cfg["bimodal_contrastive"], non_fusion_fcl=cfg["non_fusion_fcl"], fusion_combos=cfg["fusion_combos"],
             zorro=cfg["zorro"], eao=cfg["eao"], no_fusion=cfg["no_fusion"], mean_pool=cfg["mean_pool"], predrop=False, batch_dropout=True,
             epochs=1, lr=1e-3, lr_scheduler_type="cosine", num_warmup_steps=2, clip=2.0, seed=7, output_dir=str(out), dataset="unused",
             run_eval_loop=False)
    ypath = tmp_path / "drop.yaml"
    ypath.write_text(yaml.safe_dump(y, sort_keys=False))
    r = subprocess.run([sys.executable, os.path.join(REPO, "train_accel_gpu.py"), str(ypath), "--synthetic", "5", "--graph"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in open(out / "log.jsonl")]
    assert [rec["step"] for rec in recs] == [1, 2, 3, 4, 5]
    want = [float(U.draw(np.ones((4, 3), dtype=bool), list(rates.values()), 7, k, keep_one=True)[0].mean()) for k in range(5)]
    got = [rec["batch_dropout_rate"] for rec in recs]
    assert np.allclose(got, want, rtol=0, atol=1e-6), (got, want)
    assert len(set(want)) > 1 and all(rec["total_loss"] == rec["total_loss"] for rec in recs)


def test_engine_argument_errors(P):
    from torch import nn
    encs = importlib.import_module("mca-paper_amd.encoders")
    cfg = small_config("mca")
    model, _ = build(P, cfg, deterministic=False)
    eng = model.engine
    with pytest.raises(KeyError, match="smell"):
        eng.set_modality_dropout({"audio": 0.5, "smell": 0.1})
    for bad in (float("nan"), -0.1, 1.5):
        with pytest.raises(ValueError, match="video"):
            eng.set_modality_dropout({"video": bad})
    assert eng.modality_dropout is None
    eng.set_modality_dropout({"text": 1.0}, seed=7, keep_one=False)
    assert eng.modality_dropout == {"rates": {"audio": 0.0, "video": 0.0, "text": 1.0}, "seed": 7, "keep_one": False}

    class TorchSeqEncoder(nn.Module):
        def __init__(self, input_size=128, embedding_dim=512, max_tokens=1024, dropout=0.0, **kwargs):
            super().__init__()
            self.input_size, self.embedding_dim, self.max_tokens = input_size, embedding_dim, max_tokens
            self.token_encoder = nn.Sequential(nn.LayerNorm(input_size), nn.Linear(input_size, embedding_dim), nn.LayerNorm(embedding_dim))
            self.positional_encoder = encs.PositionalEncoder(embedding_dim, dropout, max_tokens)

        def forward(self, batch):
            m = batch["attention_mask"].bool()
            x = self.token_encoder(batch["tokens"].masked_fill(m[..., None], 0.0)).masked_fill(m[..., None], 0.0)
            return x + self.positional_encoder.pe[: x.shape[1]], batch["attention_mask"]

    P.encoders_dict["TorchSeqEncoder"] = TorchSeqEncoder
    try:
        cfg_f = copy.deepcopy(cfg); cfg_f["encoder_configs"]["text"]["type"] = "TorchSeqEncoder"
        foreign, _ = build(P, cfg_f, deterministic=False)
        with pytest.raises(NotImplementedError, match="native"):
            foreign.engine.set_modality_dropout({"audio": 0.5})
        foreign.engine.set_modality_dropout(None)          # switching it off is always possible
        assert foreign.engine.modality_dropout is None
    finally:
        del P.encoders_dict["TorchSeqEncoder"]
