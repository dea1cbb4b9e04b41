"""GPU tests of the gradient-cached step (mca-paper_amd/cached.py): a batch of 6 as 3 x 2 and 2 x 3 chunks against the oracle's ONE
step on the 6 samples with the assertions and tolerances of tests/test_step_gpu.py::test_small_step_vs_oracle, with both loss kernels;
the EAO model against the plain step; the n = 1 and repeat-run bitwise properties in deterministic mode; the modality dropout's draw
and counter; the finite flag of an early chunk; the refusals; and train_accel_gpu.py with grad_cache_chunks."""
import copy
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import modality_dropout_util as MU
import test_step_gpu as TS          # its tolerances and loss check: the bounds of the plain step, not of the code under test
from conftest import REPO
from util_small import small_config, rel_err, to_device, run_oracle_step

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("mca-paper_amd")


@pytest.fixture(scope="module")
def cached():
    return importlib.import_module("mca-paper_amd.cached")


optim = importlib.import_module("mca-paper_amd.optim")


def build(P, cfg, sd=None, deterministic=False, lr=1e-3, check_finite="deferred"):
    torch.manual_seed(43)
    model = P.build_model(copy.deepcopy(cfg))
    if sd is not None:
        model.load_state_dict(sd, strict=False)
    model = model.cuda()
    model.engine.check_finite = check_finite
    model.engine.set_deterministic(deterministic)
    return model, optim.FusedAdamW(model, lr=lr)


def run_cached(P, cached, cfg, sd, batch, micro_batch, kernel, lr=1e-3, clip=2.0, as_list=False):
    """util_small.run_native_step's record, from one CachedStep over the whole batch with verify on"""
    model, opt = build(P, cfg, sd, lr=lr)
    cs = cached.CachedStep(model, opt, micro_batch, clip=clip, loss_kernel=kernel, verify=True)
    dbatch = to_device(batch, "cuda")
    if as_list:
        dbatch = [cached._rows(dbatch, lo, hi) for lo, hi in cached.chunk_plan(cached._leading(dbatch), micro_batch)]
    out = cs.step(dbatch)
    model.engine.assert_finite()          # verify=True: a chunk whose second forward differed would raise here
    assert cs.last_kernel == kernel
    grads = {n: p.grad.detach().clone().cpu() for n, p in model.named_parameters()}
    by_slot = {}
    for k, sl in model.output_slots().items():
        by_slot.setdefault(sl, k)
    pooled = torch.stack([out[by_slot[sl]] for sl in sorted(by_slot)], 1)
    return dict(pooled=pooled.detach().cpu(), loss=float(out["loss"]), losses={k: float(v) for k, v in out["losses"].items()}, grads=grads,
                grad_norm=float(cs.gnorm), state={n: p.detach().clone().cpu() for n, p in model.named_parameters()}, out=out, model=model)


# ------------------------------------------------------------------------------------------------ against the oracle's one step on 6 samples
_oracle = {}


def oracle_case(P, variant, p_drop):
    """(cfg, sd, batch, fp32 oracle step, bf16-emulating oracle step) of test_small_step_vs_oracle's case, computed once"""
    key = (variant, p_drop)
    if key not in _oracle:
        from oracle import mca_oracle as O
        cfg = small_config(variant)
        batch = P.data.synthetic_batch(cfg, 6, seed=5, p_drop=p_drop)
        if variant == "tab":
            v = batch["video"]["values"]
            v[0, 3], v[1, 5], v[2, 7] = -1.0, 250.0, -10000.0
            batch["video"]["attention_mask"] = (v == -10000).to(torch.long)
        sd = P.params.init_state_dict(cfg, seed=3)
        for k in sd:
            if k.endswith("embedding.weight"):
                sd[k][::2] *= 0.05
        g = torch.Generator().manual_seed(9)
        for k in sd:
            if k.endswith("gamma") or k.endswith("bias") or ("token_encoder" in k and sd[k].dim() == 1):
                sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g)
        ref = run_oracle_step(O, cfg, sd, batch, "fp32", lr=1e-3, clip=2.0)
        emu = run_oracle_step(O, cfg, sd, batch, "bf16emu", lr=1e-3, clip=2.0)
        _oracle[key] = (cfg, sd, batch, ref, emu)
    return _oracle[key]


def check_vs_oracle(nat, ref, emu, sd):
    """every assertion of tests/test_step_gpu.py::test_small_step_vs_oracle, with its tolerances"""
    assert rel_err(nat["pooled"], ref["pooled"]) < TS.TOL_POOLED
    assert rel_err(nat["pooled"], emu["pooled"]) < TS.TOL_POOLED_EMU
    TS._check_losses(nat, ref["losses"], ref["loss"], TS._logit_scale(ref["pooled_full"]))
    errs, errs_emu = [], []
    for n, gref in ref["grads"].items():
        gn = nat["grads"][n]
        if gref.abs().max() == 0:
            assert gn.abs().max() < 1e-6, n
            continue
        e, e_emu = rel_err(gn, gref), rel_err(emu["grads"][n], gref)
        errs.append(e); errs_emu.append(e_emu)
        assert e < 4 * e_emu + 2e-2, (n, e, e_emu)
    med, med_emu = sorted(errs)[len(errs) // 2], sorted(errs_emu)[len(errs_emu) // 2]
    assert med < 1.3 * med_emu + 0.01, (med, med_emu)
    assert abs(nat["grad_norm"] - ref["grad_norm"]) < TS.TOL_GN * ref["grad_norm"]
    clip = min(1.0, 2.0 / (nat["grad_norm"] + 1e-6))
    for n, w_ref in ref["state"].items():
        upd_ref, upd_nat = w_ref - sd[n], nat["state"][n] - sd[n]
        if upd_ref.abs().max() < 1e-7:
            continue
        if not n.endswith("embedding.weight"):
            gc = nat["grads"][n].double() * clip
            want = -1e-3 * (gc / ((gc * gc).sqrt() + 1e-8)) - 1e-3 * 0.01 * sd[n].double()
            assert (upd_nat.double() - want).abs().max() < 2e-6, (n, float((upd_nat.double() - want).abs().max()))
        g_ref = ref["grads"][n]
        big = g_ref.abs() >= g_ref.abs().flatten().median()
        if int(big.sum()) >= 8:
            agree = (torch.sign(upd_nat[big]) == torch.sign(upd_ref[big])).float().mean()
            assert agree > 0.995, (n, float(agree))


@pytest.mark.parametrize("kernel", ["dense", "stream"])
@pytest.mark.parametrize("micro_batch", [2, 3])
@pytest.mark.parametrize("variant,p_drop", [("mca", 0.0), ("mca", 0.35), ("zorro", 0.35), ("tab", 0.35)])
def test_cached_step_vs_oracle_step_on_the_whole_batch(P, cached, variant, p_drop, micro_batch, kernel):
    cfg, sd, batch, ref, emu = oracle_case(P, variant, p_drop)
    nat = run_cached(P, cached, cfg, sd, batch, micro_batch, kernel, as_list=micro_batch == 3 and kernel == "dense")
    check_vs_oracle(nat, ref, emu, sd)
    # the outputs model(batch) has, for all 6 rows
    out = nat["out"]
    assert out["loss"].shape == () and all(v.shape == (6,) and v.dtype == torch.bool for v in out["modality_sample_mask"].values())
    assert ("fcl_loss" in out) == (cfg["fcl"] and not cfg["zorro"]) and "modality_dropped" not in out
    for name in cfg["encoder_configs"]:
        am = batch[name]["attention_mask"].bool()
        assert torch.equal(out["modality_sample_mask"][name].cpu(), ~am.all(1)), name


def test_big_batch_loss_is_not_the_mean_of_the_chunk_losses(P, cached):
    """with missing modalities n_{t,r} counts over all 6 rows and the negatives are all 6: a step that averaged the losses of the
    chunks would be seen by the test above"""
    cfg, sd, batch, ref, _ = oracle_case(P, "mca", 0.35)
    model, _ = build(P, cfg, sd)
    dbatch = to_device(batch, "cuda")
    per = []
    with torch.no_grad():
        for lo, hi in cached.chunk_plan(6, 2):
            per.append({k: float(v) for k, v in model(cached._rows(dbatch, lo, hi))["losses"].items()})
    tol = TS.TOL_LOGIT * TS._logit_scale(ref["pooled_full"]) + 1e-4
    far = []
    for k, v in ref["losses"].items():
        vals = [p[k] for p in per if p[k] == p[k]]
        if float(v) == float(v) and vals:
            far.append(abs(sum(vals) / len(vals) - float(v)) > tol)
    assert any(far), "the chunk-wise mean is within the test's tolerance of the whole-batch loss: the case shows nothing"


def test_eao_cached_step_against_the_plain_step(P, cached):
    """the bounds tests/test_graph_gpu.py allows between an eager and a replayed step from one state: 1e-5 of the loss (its first step,
    before any drift), 2e-3 of the gradient norm and 5e-3 of the flat gradient (its one-step comparison at CMU size)"""
    cfg = small_config("eao")
    sd = P.params.init_state_dict(cfg, seed=3)
    batch = to_device(P.data.synthetic_batch(cfg, 4, seed=5, p_drop=0.35), "cuda")
    plain, opt = build(P, cfg, sd)
    out = plain(batch)
    opt.zero_grad()
    out["loss"].backward()
    gn = float(optim.clip_grad_norm_(plain, 2.0))
    opt.step()
    for kernel in ("dense", "stream"):
        model, o2 = build(P, cfg, sd)
        cs = cached.CachedStep(model, o2, 2, clip=2.0, loss_kernel=kernel, verify=True)
        got = cs.step(batch)
        model.engine.assert_finite()
        le, lg = float(out["loss"]), float(got["loss"])
        print(f"eao cached ({kernel}) against plain: loss {le!r} / {lg!r} rel {abs(le - lg) / abs(le):.2e}, gnorm rel {abs(gn - float(cs.gnorm)) / gn:.2e}, "
              f"gflat {rel_err(model.engine.gflat, plain.engine.gflat):.2e}, weights {rel_err(model.engine.flat, plain.engine.flat):.2e}")
        assert abs(le - lg) <= 1e-5 * abs(le), (kernel, le, lg)
        assert abs(gn - float(cs.gnorm)) <= 2e-3 * gn and rel_err(model.engine.gflat, plain.engine.gflat) < 5e-3, kernel
        assert rel_err(model.engine.flat, plain.engine.flat) <= 1e-3, kernel
        assert set(got["losses"]) == set(out["losses"])


# ------------------------------------------------------------------------------------------------ bitwise properties
def test_one_chunk_dense_is_forward_backward_bit_for_bit(P, cached):
    cfg = small_config("mca")
    sd = P.params.init_state_dict(cfg, seed=3)
    batch = to_device(P.data.synthetic_batch(cfg, 4, seed=5, p_drop=0.35), "cuda")
    a, _ = build(P, cfg, sd, deterministic=True)
    out = a.engine.forward_backward(batch)
    b, ob = build(P, cfg, sd, deterministic=True)
    cs = cached.CachedStep(b, ob, 4, clip=2.0, loss_kernel="dense", verify=True)
    got = cs.step(batch)
    torch.cuda.synchronize()
    assert torch.equal(a.engine.gflat, b.engine.gflat) and float(a.engine.gflat.abs().max()) > 0
    assert torch.equal(out["loss"], got["loss"])


@pytest.mark.parametrize("kernel", ["dense", "stream"])
def test_two_runs_from_one_state_give_the_same_bits(P, cached, kernel):
    cfg = small_config("tab")
    sd = P.params.init_state_dict(cfg, seed=3)
    batch = to_device(P.data.synthetic_batch(cfg, 6, seed=5, p_drop=0.35), "cuda")
    res = []
    for _ in range(2):
        m, o = build(P, cfg, sd, deterministic=True)
        cs = cached.CachedStep(m, o, 2, clip=2.0, loss_kernel=kernel, verify=True)
        out = cs.step(batch)
        m.engine.assert_finite()
        res.append((out["loss"].clone(), m.engine.gflat.clone(), m.engine.flat.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert not torch.equal(res[0][2], build(P, cfg, sd)[0].engine.flat)          # the step did move the weights


# ------------------------------------------------------------------------------------------------ modality dropout
def test_chunks_draw_the_rows_of_the_one_step_draw_and_the_counter_moves_once(P, cached):
    cfg = small_config("mca")
    M, SEED = len(cfg["encoder_configs"]), 42
    batch = to_device(P.data.synthetic_batch(cfg, 8, seed=5, p_drop=0.0), "cuda")
    model, opt = build(P, cfg)
    model.train()
    model.engine.set_modality_dropout({n: 0.5 for n in model.modality_types}, seed=SEED, keep_one=True, step=3)
    cs = cached.CachedStep(model, opt, 2, clip=2.0, verify=True)
    for t in (3, 4):
        out = cs.step(batch)
        model.engine.assert_finite()
        want, _, _ = MU.draw(np.ones((8, M), dtype=bool), [0.5] * M, SEED, t, keep_one=True)          # the plain step's draw on 8 samples
        assert want.any() and not want.all()
        assert np.array_equal(out["modality_dropped"].cpu().numpy(), want), t
        assert model.engine.modality_dropout_step() == t + 1
        for i, n in enumerate(model.modality_types):
            assert np.array_equal(out["modality_sample_mask"][n].cpu().numpy(), ~want[:, i])
    # and the plain step on the same 8 samples at the same counter value draws that matrix
    plain, _ = build(P, cfg)
    plain.train()
    plain.engine.set_modality_dropout({n: 0.5 for n in plain.modality_types}, seed=SEED, keep_one=True, step=4)
    with torch.no_grad():
        assert torch.equal(plain(batch)["modality_dropped"], out["modality_dropped"])


# ------------------------------------------------------------------------------------------------ flags and refusals
def test_nan_in_the_first_chunk_skips_the_update(P, cached):
    cfg = small_config("mca")
    batch = to_device(P.data.synthetic_batch(cfg, 6, seed=5, p_drop=0.0), "cuda")
    batch["audio"]["tokens"][0, 0, 0] = float("nan")
    model, opt = build(P, cfg, check_finite="deferred")
    w0, m0, v0 = model.engine.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    cs = cached.CachedStep(model, opt, 2, clip=2.0)
    cs.step(batch)
    torch.cuda.synchronize()
    assert torch.equal(model.engine.flat, w0) and torch.equal(opt.exp_avg, m0) and torch.equal(opt.exp_avg_sq, v0)
    with pytest.raises(Exception, match="not finite"):
        model.engine.assert_finite()


def test_verify_sees_a_second_forward_that_differs(P, cached, monkeypatch):
    """a weight moved between the passes (planted in the loss call): chunk 0's second forward gives other pooled tokens; with verify
    the update is skipped and the next poll raises, without it the step goes through"""
    cfg = small_config("mca")
    batch = to_device(P.data.synthetic_batch(cfg, 4, seed=5, p_drop=0.0), "cuda")
    for verify in (True, False):
        model, opt = build(P, cfg)
        eng = model.engine
        inner = eng.loss_fwd_bwd_bank

        def moved(bank, present, kernel, eng=eng, inner=inner):
            res = inner(bank, present, kernel)
            model.return_tokens.data.add_(0.01)
            eng.invalidate_weights()
            return res

        monkeypatch.setattr(eng, "loss_fwd_bwd_bank", moved)
        cs = cached.CachedStep(model, opt, 2, clip=2.0, verify=verify)
        cs.step(batch)
        torch.cuda.synchronize()
        before = opt.exp_avg.clone()
        if verify:
            assert float(opt.exp_avg.abs().max()) == 0.0          # the optimizer left its state alone
            with pytest.raises(RuntimeError, match="did not reproduce"):
                eng.assert_finite()
        else:
            eng.assert_finite()
            assert float(before.abs().max()) > 0.0


def test_refusals_raise_before_anything_is_launched(P, cached, monkeypatch):
    cfg = small_config("mca")
    model, opt = build(P, cfg)
    batch = to_device(P.data.synthetic_batch(cfg, 6, seed=5), "cuda")
    hip = importlib.import_module("mca-paper_amd.hip")
    launched = []
    for mod in (hip, cached, importlib.import_module("mca-paper_amd.engine"), optim):          # every module that launches by name
        monkeypatch.setattr(mod, "call", lambda *a, **k: launched.append(a[0]))
    with pytest.raises(ValueError, match="no positive multiple of micro_batch = 4"):
        cached.CachedStep(model, opt, 4).step(batch)
    with pytest.raises(ValueError, match="loss_kernel"):
        cached.CachedStep(model, opt, 2, loss_kernel="fast")
    with pytest.raises(NotImplementedError, match="data-parallel"):
        cached.CachedStep(model, opt, 2, dp=object())
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE = 2"):
        cached.CachedStep(model, opt, 2)
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setattr(model.engine, "can_forward_backward", lambda: False)
    with pytest.raises(NotImplementedError, match="native encoders"):
        cached.CachedStep(model, opt, 2)
    monkeypatch.undo()
    assert launched == []
    graph = importlib.import_module("mca-paper_amd.graph")
    g = graph.GraphedStep(model, opt, cached._rows(batch, 0, 2), clip=2.0)
    with pytest.raises(RuntimeError, match="GraphedStep"):
        cached.CachedStep(model, opt, 2)
    del g


# ------------------------------------------------------------------------------------------------ the training script
def test_train_script_with_grad_cache_chunks(P, cached, tmp_path):
    """--synthetic 4 with grad_cache_chunks: 2: two optimizer steps per epoch over 2 x batch_size samples, the usual record keys;
    together with --graph the run ends with a message that names both"""
    import yaml
    cfg = small_config("mca")
    mod_cfg = {name: {"type": "embedded_sequence", "pad_len": enc["max_tokens"], "embedding_size": enc["input_size"], "data_col_name": "data", "dropout": 0.2}
               for name, enc in cfg["encoder_configs"].items()}

    def run(tag, extra, **keys):
        out = tmp_path / tag
        y = dict(encoder_configs=cfg["encoder_configs"], modality_config=mod_cfg, hidden_size=cfg["dim"], layers=cfg["depth"], heads=cfg["heads"],
                 dim_head=cfg["dim_head"], num_fusion_tokens=cfg["num_fusion_tokens"], batch_size=4, fcl=cfg["fcl"], fcl_root=cfg["fcl_root"],
                 bimodal_contrastive=cfg["bimodal_contrastive"], non_fusion_fcl=cfg["non_fusion_fcl"], fusion_combos=cfg["fusion_combos"],
                 zorro=cfg["zorro"], eao=cfg["eao"], no_fusion=cfg["no_fusion"], mean_pool=cfg["mean_pool"], predrop=True, epochs=1, lr=1e-3,
                 lr_scheduler_type="cosine", num_warmup_steps=1, clip=2.0, seed=7, output_dir=str(out), dataset="unused", run_eval_loop=False, **keys)
        ypath = tmp_path / f"{tag}.yaml"
        ypath.write_text(yaml.safe_dump(y, sort_keys=False))
        r = subprocess.run([sys.executable, os.path.join(REPO, "train_accel_gpu.py"), str(ypath), "--synthetic", "4"] + extra,
                           capture_output=True, text=True, timeout=600)
        return r, out

    r, out = run("cached", ["--deterministic"], grad_cache_chunks=2)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in open(out / "log.jsonl")]
    assert [rec["step"] for rec in recs] == [1, 2]
    # every step consumed ITS two loader batches: the same model and schedule here, one CachedStep per step on synthetic batches
    # (0, 1) then (2, 3), built as the script builds them.  The same kernels on the same data: the one-step allowance of
    # tests/test_graph_gpu.py between two runs of a step, 1e-6 of the loss.  Batches (0, 0) would miss it by far.
    train = importlib.import_module("train_accel_gpu")
    config = P.config.training_config(str(tmp_path / "cached.yaml"), make_output_dir=False)
    model_config = P.config.get_model_config(config)

    def fresh():
        torch.manual_seed(config.seed)
        model = P.build_model(model_config).cuda()
        opt = optim.FusedAdamW(model, lr=config.lr)
        model.engine.check_finite = "deferred"
        model.engine.set_deterministic(True)
        model.train()
        return model, opt, cached.CachedStep(model, opt, config.batch_size, clip=config.clip)

    model, opt, cs = fresh()
    host = [P.data.synthetic_batch(model_config, config.batch_size, seed=1234 + 1000 * i, p_drop=0.2) for i in range(4)]
    got = []
    for st in range(2):
        for g in opt.param_groups:
            g["lr"] = config.lr * train.lr_factor(config.lr_scheduler_type, st, config.num_warmup_steps, 2)
        got.append(float(cs.step([to_device(host[2 * st], "cuda"), to_device(host[2 * st + 1], "cuda")])["loss"]))
    model.engine.assert_finite()
    print("script losses", [rec["total_loss"] for rec in recs], "CachedStep on batches (0, 1), (2, 3)", got)
    for rec, want in zip(recs, got):
        assert abs(rec["total_loss"] - want) <= 1e-6 * abs(want), (rec["total_loss"], want)
    aliased = float(fresh()[2].step([to_device(host[0], "cuda")] * 2)["loss"])
    assert abs(aliased - got[0]) > 1e-3 * abs(got[0]), "a step on batch 0 twice is not told from the step on batches 0 and 1: the check shows nothing"
    r1, out1 = run("plain", [])
    assert r1.returncode == 0, r1.stderr[-3000:]
    plain = [json.loads(l) for l in open(out1 / "log.jsonl")]
    assert [rec["step"] for rec in plain] == [1, 2, 3, 4] and set(recs[0]) == set(plain[0])
    for rec in recs:
        assert all(v == v and abs(v) < 1e9 for v in rec.values() if isinstance(v, float)), rec
    assert os.path.exists(out / "0" / "model.safetensors") and os.path.exists(out / "0" / "optimizer.bin")
    r2, _ = run("refused", ["--graph"], grad_cache_chunks=2)
    assert r2.returncode != 0 and "grad_cache_chunks" in r2.stderr and "--graph" in r2.stderr
