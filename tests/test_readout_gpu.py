"""GPU tests of the attention readout: mca_attn_readout through the C ABI against the dense fp64 softmax of the same bf16
operands (model.py:87-99 restated, log2 domain), and MCA.attention_readout / infer_accel_gpu.py --readout on small models.

The bound on every mass and probability entry is derived, not tuned:
    |got - ref| <= 2 * tol * ref + 1e-7,   tol = ln 2 * (e_lse + 2 * 64 * 2^-24 * max_ij sum_d |q_id k_jd|) + 4 * 2^-24
e_lse: distance of the log-sum-exp the kernel was given from the fp64 one (measured per case: the forward's, or 2^-24 max|lse| when
the fp64 value rounded to fp32 is fed in, which isolates the readout kernel); the middle term is the fp32 accumulation of 64 exact
bf16 products, the last one the rounding of exp2.  Each case prints the largest observed ratio to that bound (pytest -s).

One deliberate reading of "the dropped modality's column is 0.0 for that sample": it holds for every slot whose pooling row is not
fully masked.  The dropped modality's OWN slot is a fully masked row, which by the same contract reads as the uniform shares."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from util_small import small_config, rel_err, to_device

pytestmark = pytest.mark.gpu
C2 = 0.125 * 1.4426950408889634          # scale * log2(e), folded into the stored q
LN2 = 0.6931471805599453
U = 2.0 ** -24
DEV = "cuda"


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def bf(x):
    return x.to(torch.bfloat16)


def dense_probs(q_st, k_st, allowed, pad):
    """softmax of model.py:87-99 in fp64 from the STORED operands (q already carries scale * log2 e: q.k is the log2-domain logit).
    q_st (b,h,nq,64), k_st (b,h,nk,64), allowed (nq,nk) bool, pad (b,nk) bool -> P (b,h,nq,nk), lse (b,h,nq; 0 on uniform rows),
    uni (b,nq) bool.  A fully masked row is uniform over all nk keys (softmax of a constant row)."""
    s = torch.einsum("bhid,bhjd->bhij", q_st.double(), k_st.double())
    blocked = (~allowed)[None, None] | pad[:, None, None, :]          # (b,1,nq,nk)
    uni = blocked.all(-1)[:, 0]                                        # (b,nq)
    s = s.masked_fill(blocked, float("-inf"))
    lse = torch.logsumexp(s * LN2, -1) / LN2
    lse = torch.where(uni[:, None, :], torch.zeros_like(lse), lse)
    P = torch.exp2(s - lse[..., None])
    P = torch.where(uni[:, None, :, None], torch.full_like(P, 1.0 / s.shape[-1]), P)
    return P, lse, uni


def group_sums(P, kgroup, G):
    return torch.stack([P[..., kgroup == g].sum(-1) for g in range(G)], -1)


CASES = {}
for _z in (False, True):
    for _pool in (False, True):
        for _drop in (False, True):
            CASES[f"s3-{'zorro' if _z else 'fcl'}-{'pool' if _pool else 'layer'}{'-drop' if _drop else ''}"] = dict(
                dims=[70, 45, 30], F=8, powers=(3, 2), zorro=_z, b=3, heads=2, pool=_pool, drop=_drop)
CASES["g15-layer"] = dict(dims=[40, 30, 20, 10], F=33, powers=(4, 3, 2), zorro=False, b=2, heads=2, pool=False, drop=True)
CASES["g21-layer"] = dict(dims=[40, 30, 20, 10, 24], F=32, powers=(5, 4, 3), zorro=False, b=2, heads=2, pool=False, drop=True)
CASES["g21-pool"] = dict(dims=[40, 30, 20, 10, 24], F=32, powers=(5, 4, 3), zorro=False, b=2, heads=2, pool=True, drop=False)
CASES["spike-layer"] = dict(dims=[300, 100, 60], F=8, powers=(3, 2), zorro=False, b=2, heads=2, pool=False, drop=False, spike=True)
CASES["cmu-layer"] = dict(dims=[1500, 450, 450, 50], F=88, powers=(4, 3, 2), zorro=False, b=1, heads=2, pool=False, drop=False)
_BUILT = {}


class Case:
    pass


def build_case(H, name):
    """operands, masks and padding as tests/test_attention_gpu.py builds them; the forward's lse; the fp64 reference (once per case)"""
    if name in _BUILT:
        return _BUILT[name]
    p = CASES[name]
    S = importlib.import_module("mca-paper_amd.structure")
    A = importlib.import_module("mca-paper_amd.attention")
    RO = importlib.import_module("mca-paper_amd.readout")
    c = Case()
    st = S.FusionStructure(p["dims"], p["F"], p["powers"], fcl=not p["zorro"], zorro=p["zorro"])
    b, heads, pool = p["b"], p["heads"], p["pool"]
    N, D = st.n_tokens, heads * 64
    g = torch.Generator(device=DEV).manual_seed(7)
    qmask_np = st.qmask_pool if pool else st.qmask_attn
    nq = len(qmask_np)
    c.st, c.b, c.heads, c.N, c.D, c.nq, c.pool, c.G = st, b, heads, N, D, nq, pool, st.n_groups
    c.sf = A._Sched(st.pool_schedule(128, 64) if pool else st.attn_schedule(128, 64), DEV)
    c.qmask = torch.from_numpy(qmask_np.astype(np.uint32).view(np.int32)).to(DEV)
    c.qbits = torch.from_numpy(((qmask_np[:, None].astype(np.int64) >> np.arange(c.G)[None, :]) & 1).astype(bool)).to(DEV)          # (nq, G)
    c.kgroup = torch.from_numpy(st.kgroup).to(DEV)
    c.allowed = torch.from_numpy(~(st.dense_pool_mask() if pool else st.dense_attn_mask())).to(DEV)
    pad = torch.zeros(b, N, dtype=torch.bool, device=DEV)
    off = 0
    for mi, n in enumerate(st.token_dims):
        ln = torch.randint(1, n + 1, (b,), generator=g, device=DEV)
        if p["drop"] and mi == 0:
            ln[0] = 0
        pad[:, off:off + n] = torch.arange(n, device=DEV)[None] >= ln[:, None]
        off += n
    c.pad = pad
    qkv = torch.randn(b, N, 3 * D, device=DEV, generator=g)
    if p.get("spike"):
        for j in (3, 70, 131, N - 2):
            qkv[:, j, D:2 * D] *= 40.0
    qkv = bf(qkv)
    if pool:
        c.qsrc = bf(torch.randn(nq, D, device=DEV, generator=g) * C2)
        q_st = c.qsrc.view(1, nq, heads, 64).permute(0, 2, 1, 3).expand(b, -1, -1, -1)
    else:
        qkv[:, :, :D] = bf(qkv[:, :, :D].float() * C2)
        q_st = qkv[:, :, :D].view(b, N, heads, 64).permute(0, 2, 1, 3)
    c.qkv = qkv
    k_st = qkv[:, :, D:2 * D].view(b, N, heads, 64).permute(0, 2, 1, 3)
    c.P, c.lse_ref, c.uni = dense_probs(q_st, k_st, c.allowed, pad)
    c.mass_ref = group_sums(c.P, c.kgroup, c.G)
    c.maxdot = float(torch.einsum("bhid,bhjd->bhij", q_st.double().abs(), k_st.double().abs()).max())
    c.um = torch.from_numpy(RO.uniform_mass(st)).to(DEV)
    c.inv_nk = float(np.float32(1.0) / np.float32(N))

    c.nk_pad = (N + 255) // 256 * 256
    c.keyinfo = torch.empty(b, c.nk_pad, dtype=torch.uint8, device=DEV)
    c.kflags = torch.empty(b, (N + 63) // 64, dtype=torch.uint8, device=DEV)
    H.call("mca_build_keyinfo", pad.to(torch.uint8).data_ptr(), c.kgroup.data_ptr(), c.keyinfo.data_ptr(), c.kflags.data_ptr(), b, N, c.nk_pad,
           H.stream_ptr())
    vmean = torch.empty(b, D, device=DEV)
    vptr = qkv.data_ptr() + 2 * D * 2
    H.call("mca_attn_vmean", vptr, N * 3 * D, 3 * D, vmean.data_ptr(), b, N, heads, H.stream_ptr())
    o = torch.zeros(b * nq, D, dtype=torch.bfloat16, device=DEV)
    c.lse = torch.empty(b, heads, nq, device=DEV)
    c.A = A
    c.keys = A.AttnKeys(c.keyinfo, c.kflags, None, N, c.nk_pad, b, heads, 0.125, H.ATTN_Q_PRESCALED)
    c.ops = A.AttnOperands(c.qsrc.data_ptr() if pool else qkv.data_ptr(), 0 if pool else N * 3 * D, D if pool else 3 * D, qkv, D, 2 * D, 3 * D,
                           o, c.lse, nq, c.qmask, None, c.sf, None, None)
    H.call("mca_attn_fwd", C.byref(A.fwd_args(c.ops, c.keys, vmean)), H.stream_ptr())
    torch.cuda.synchronize()
    # the forward marks exactly the dense reference's uniform rows, and its lse is the dense one (the forward test's bound)
    assert torch.equal(torch.isinf(c.lse), c.uni[:, None, :].expand(-1, heads, -1))
    fin = ~torch.isinf(c.lse)
    c.e_lse_fwd = float((c.lse[fin].double() - c.lse_ref[fin]).abs().max()) if fin.any() else 0.0
    assert c.e_lse_fwd < 1e-3
    # the fp64 lse rounded to fp32 (+inf on uniform rows): isolates the readout kernel
    c.lse64 = torch.where(c.uni[:, None, :], torch.full_like(c.lse_ref, float("inf")), c.lse_ref).float().contiguous()
    c.e_lse_64 = U * float(c.lse_ref.abs().max())
    _BUILT[name] = c
    return c


def readout_args(H, c, lse, mass, probs=None, row0=0, n_rows=0):
    assert probs is None or n_rows == probs.shape[2]
    return c.A.readout_args(c.ops._replace(lse=lse), c.keys, c.um, mass, probs, row0)


def run_readout(H, c, lse, window=None):
    """-> (mass, probs or None); both outputs are NaN before the launch"""
    mass = torch.full((c.b, c.heads, c.nq, c.G), float("nan"), device=DEV)
    probs = None
    if window is not None:
        probs = torch.full((c.b, c.heads, window[1], c.N), float("nan"), device=DEV)
    a = readout_args(H, c, lse, mass, probs, *(window or (0, 0)))
    H.call("mca_attn_readout", C.byref(a), H.stream_ptr())
    torch.cuda.synchronize()
    return mass, probs


def bound_ratio(got, ref, tol):
    """largest |got - ref| / (2 tol ref + 1e-7)"""
    return float(((got.double() - ref).abs() / (2.0 * tol * ref + 1e-7)).max())


def windows_of(c):
    """the probs windows of a case: the whole pooling query; else the fusion-token rows (they cross the 128-row tile edge where
    N - F < 128 < N) and one row at an odd row0"""
    if c.pool:
        return [(0, c.nq)]
    F = c.st.num_fusion_tokens
    return [(c.N - F, F), (min(131, c.N - 2) | 1, 1)]


def check_outputs(c, mass, probs, window, tol, tag):
    uni_h = c.uni[:, None, :].expand(-1, c.heads, -1)          # (b,h,nq)
    assert not torch.isnan(mass).any(), "mass: an element was not written"
    r_mass = bound_ratio(mass, c.mass_ref, tol)
    line = f"READOUT_RATIO {tag} tol={2 * tol:.3e} mass={r_mass:.4f}"
    # ---- exactness
    assert torch.equal(mass[uni_h], c.um[None].expand(int(uni_h.sum()), -1)), "uniform rows: mass is not uniform_mass bit for bit"
    assert torch.equal((mass == c.um).all(-1), uni_h), "the rows that read as uniform are not the dense reference's"
    nonuni = ~uni_h
    blocked_g = ~c.qbits[None, None].expand(c.b, c.heads, -1, -1)          # (b,h,nq,G)
    assert (mass[blocked_g & nonuni[..., None]] == 0.0).all(), "a group the row's qmask blocks has mass"
    valid_per_group = torch.stack([((c.kgroup == g)[None] & ~c.pad).any(-1) for g in range(c.G)], -1)          # (b,G)
    allpad = (~valid_per_group)[:, None, None, :].expand(-1, c.heads, c.nq, -1)
    assert (mass[allpad & nonuni[..., None]] == 0.0).all(), "a group whose keys are all padded has mass"
    # ---- every non-uniform row sums to 1
    sums = mass.double().sum(-1)[nonuni]
    if sums.numel():
        assert float((sums - 1.0).abs().max()) <= 2 * tol + c.G * 1e-7, float((sums - 1.0).abs().max())
    if probs is not None:
        r0, n = window
        assert not torch.isnan(probs).any(), "probs: an element was not written"
        Pw = c.P[:, :, r0:r0 + n]
        r_probs = bound_ratio(probs, Pw, tol)
        line += f" probs={r_probs:.4f}"
        uw = uni_h[:, :, r0:r0 + n]
        dead = ((~c.allowed)[None, None, r0:r0 + n] | c.pad[:, None, None, :]).expand(-1, c.heads, -1, -1) & ~uw[..., None]
        assert (probs[dead] == 0.0).all(), "a padded or blocked key has probability"
        if uw.any():
            assert (probs[uw] == torch.tensor(c.inv_nk, device=DEV)).all(), "uniform rows: probs is not 1 / nk bit for bit"
        # probs summed by group is the mass (fp32 summation error)
        d = (group_sums(probs.double(), c.kgroup, c.G) - mass[:, :, r0:r0 + n].double()).abs().max()
        assert float(d) <= 4 * c.N * U, float(d)
        assert r_probs <= 1.0, line
    print(line, flush=True)
    assert r_mass <= 1.0, line


@pytest.mark.parametrize("name", list(CASES))
def test_readout_kernel_against_dense_fp64(H, name):
    c = build_case(H, name)
    tol_fwd = LN2 * (c.e_lse_fwd + 2 * 64 * U * c.maxdot) + 4 * U
    tol_64 = LN2 * (c.e_lse_64 + 2 * 64 * U * c.maxdot) + 4 * U
    wins = windows_of(c)
    # with the forward's lse, first window; twice: the same bits, every element written (NaN before each launch)
    m1, p1 = run_readout(H, c, c.lse, wins[0])
    m2, p2 = run_readout(H, c, c.lse, wins[0])
    assert torch.equal(m1, m2) and torch.equal(p1, p2), "two launches differ"
    check_outputs(c, m1, p1, wins[0], tol_fwd, f"{name} lse=forward e_lse={c.e_lse_fwd:.2e} window={wins[0]}")
    # without probs: the same mass
    m3, _ = run_readout(H, c, c.lse, None)
    assert torch.equal(m1, m3)
    # with the fp64 lse: the kernel alone
    for w in wins[::-1]:
        m4, p4 = run_readout(H, c, c.lse64, w)
        check_outputs(c, m4, p4, w, tol_64, f"{name} lse=fp64 e_lse={c.e_lse_64:.2e} window={w}")


def test_readout_refusals_leave_outputs_untouched(H):
    c = build_case(H, "s3-fcl-layer")
    lib = H.lib()
    mass = torch.full((c.b, c.heads, c.nq, c.G), -7.0, device=DEV)
    probs = torch.full((c.b, c.heads, 4, c.N), -7.0, device=DEV)

    def rc(mut, with_probs=False):
        a = readout_args(H, c, c.lse, mass, probs if with_probs else None, 3, 4)
        mut(a)
        return lib.mca_attn_readout(C.byref(a), H.stream_ptr())

    for field in ("q", "k", "lse", "qmask", "keyinfo", "ktile_flags", "q_ptr", "q_kt", "q_order", "uniform_mass", "mass"):
        assert rc(lambda a: setattr(a, field, None)) == -1, field
    assert lib.mca_attn_readout(None, H.stream_ptr()) == -1
    for G in (0, -1, 32):
        assert rc(lambda a: setattr(a, "n_groups", G)) == -1, G
    for row0, n in ((-1, 4), (c.nq, 1), (c.nq - 3, 4), (0, 0), (0, c.nq + 1), (5, -2)):
        def win(a):
            a.row0, a.n_rows = row0, n
        assert rc(win, with_probs=True) == -1, (row0, n)
    assert rc(lambda a: setattr(a, "flags", 0)) == -3
    assert rc(lambda a: setattr(a, "flags", H.ATTN_LAZY_REFERENCE)) == -3
    torch.cuda.synchronize()
    assert (mass == -7.0).all() and (probs == -7.0).all()
    # (the window is read only when probs is given)
    assert rc(lambda a: setattr(a, "row0", -5)) == 0
    torch.cuda.synchronize()
    assert not (mass == -7.0).any() and (probs == -7.0).all()


# ---------------------------------------------------------------------------------------------- model level
def _model_case(variant):
    P = importlib.import_module("mca-paper_amd")
    cfg = small_config(variant, depth=2)
    torch.manual_seed(3)
    model = P.build_model(cfg).to(DEV).eval()
    batch = P.data.synthetic_batch(cfg, 4, seed=11)
    batch["audio"]["attention_mask"][1] = True          # sample 1 loses its first modality
    batch["audio"]["tokens"][1] = 0.0
    return P, cfg, model, to_device(batch, DEV)


@pytest.mark.parametrize("variant", ["mca", "zorro"])
def test_model_readout_matches_dense_formula_on_saved_operands(H, variant):
    P, cfg, model, batch = _model_case(variant)
    RO = importlib.import_module("mca-paper_amd.readout")
    eng = model.engine
    b, Hh, N, R, D, F = 4, eng.H, eng.N, eng.R, eng.D, eng.F
    before = model(batch, no_loss=True)
    before = {k: v.clone() for k, v in before.items() if torch.is_tensor(v)}
    ro = model.attention_readout(batch, probs_rows={"pool": (0, R), 0: (N - F, F), 1: (33, 1)})
    torch.cuda.synchronize()
    ws = eng.workspace(b)
    G = eng.st.n_groups
    assert ro["groups"] == RO.group_names(model) and len(ro["groups"]) == G
    assert set(ro["layer_mass"]) == {0, 1} and set(ro["probs"]) == {"pool", 0, 1}
    pad = torch.cat([batch[m]["attention_mask"].bool() for m in model.modality_types] + [torch.zeros(b, F, dtype=torch.bool, device=DEV)], 1)
    assert torch.equal(pad, ws["padding"].view(b, N).bool())
    kgroup = torch.from_numpy(eng.st.kgroup).to(DEV)
    um = torch.from_numpy(RO.uniform_mass(eng.st)).to(DEV)

    def check(q_st, k_st, blocked_mask, lse_saved, mass, probs, window, tag):
        Pd, lse_ref, uni = dense_probs(q_st, k_st, ~blocked_mask, pad)
        fin = ~torch.isinf(lse_saved)
        assert torch.equal(~fin, uni[:, None, :].expand(-1, Hh, -1))
        e_lse = float((lse_saved[fin].double() - lse_ref[fin]).abs().max())
        assert e_lse < 1e-3
        maxdot = float(torch.einsum("bhid,bhjd->bhij", q_st.double().abs(), k_st.double().abs()).max())
        tol = LN2 * (e_lse + 2 * 64 * U * maxdot) + 4 * U
        rm = bound_ratio(mass, group_sums(Pd, kgroup, G), tol)
        r0, n = window
        rp = bound_ratio(probs, Pd[:, :, r0:r0 + n], tol)
        print(f"READOUT_RATIO model-{variant}-{tag} tol={2 * tol:.3e} mass={rm:.4f} probs={rp:.4f}", flush=True)
        assert rm <= 1.0 and rp <= 1.0, (tag, rm, rp)
        uni_h = uni[:, None, :].expand(-1, Hh, -1)
        assert torch.equal(mass[uni_h], um[None].expand(int(uni_h.sum()), -1))
        return uni, tol

    for i, win in ((0, (N - F, F)), (1, (33, 1))):
        qkv = ws["layers"][i]["qkv"].view(b, N, 3 * D)
        q_st = qkv[:, :, :D].view(b, N, Hh, 64).permute(0, 2, 1, 3)
        k_st = qkv[:, :, D:2 * D].view(b, N, Hh, 64).permute(0, 2, 1, 3)
        uni, _ = check(q_st, k_st, model.attn_mask, ws["layers"][i]["lse"], ro["layer_mass"][i], ro["probs"][i], win, f"layer{i}")
        assert uni[1, :70].all() and not uni[0].any()          # the dropped modality's own rows are fully masked
    kvp = ws["kvp"].view(b, N, 2 * D)
    q_st = ws["qp"].view(1, R, Hh, 64).permute(0, 2, 1, 3).expand(b, -1, -1, -1)
    k_st = kvp[:, :, :D].view(b, N, Hh, 64).permute(0, 2, 1, 3)
    uni_p, tol_p = check(q_st, k_st, model.pool_mask, ws["lse_p"], ro["pool_mass"], ro["probs"]["pool"], (0, R), "pool")
    # probs @ V per head is the pooling attention's saved output (the forward test's bound)
    v_st = kvp[:, :, D:].view(b, N, Hh, 64).permute(0, 2, 1, 3).float()
    o = torch.einsum("bhij,bhjd->bhid", ro["probs"]["pool"], v_st).permute(0, 2, 1, 3).reshape(b * R, D)
    assert rel_err(ws["op"].float(), o) < 6e-3, rel_err(ws["op"].float(), o)
    # slot_mass: the head mean of the slot's row; rows sum to 1; blocked groups and the dropped modality read 0.0
    slots = model.output_slots()
    assert set(ro["slot_mass"]) == set(slots)
    pool_blocked = model.pool_mask          # (R, N) True = blocked
    for k, row in slots.items():
        sm = ro["slot_mass"][k]
        assert sm.shape == (b, G)
        assert torch.equal(sm, ro["pool_mass"][:, :, row].mean(1))
        assert float((sm.double().sum(-1) - 1.0).abs().max()) <= 2 * tol_p + G * 1e-7          # (uniform rows: the fp32 shares, G * 2^-24)
        for s in range(b):
            if uni_p[s, row]:          # a fully masked pooling row (the dropped modality's own slot): the uniform shares
                assert s == 1 and k == "audio" and torch.equal(sm[s], um)
                continue
            for g in range(G):
                if bool(pool_blocked[row][kgroup == g].all()):
                    assert float(sm[s, g]) == 0.0, (k, s, g)
            if s == 1:
                assert float(sm[s, 0]) == 0.0, (k, "the dropped modality's column")
    assert bool(uni_p[1, slots["audio"]])
    assert not ro["modality_sample_mask"]["audio"][1] and ro["modality_sample_mask"]["audio"][0]
    # the forward is untouched: the same bits before and after a readout
    after = model(batch, no_loss=True)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k


def test_model_readout_refuses_fp8_attention_engines(H):
    P, cfg, model, batch = _model_case("mca")
    model.engine.set_attention_dtype("fp8")
    with pytest.raises(NotImplementedError, match="fp8"):
        model.attention_readout(batch)


def test_infer_script_readout_flag(H, tmp_path):
    """infer_accel_gpu.py --synthetic 2 with and without --readout: the new file's keys and shapes, its slot_mass against the
    method's on the same model and batches, and the six old files byte for byte."""
    import yaml
    P = importlib.import_module("mca-paper_amd")
    cfg = small_config("mca")
    mod_cfg = {name: {"type": "embedded_sequence", "pad_len": enc["max_tokens"], "embedding_size": enc["input_size"], "data_col_name": "data", "dropout": 0.0}
               for name, enc in cfg["encoder_configs"].items()}
    old = [f"{tv}_{what}.pt" for tv in ("train", "eval") for what in ("embeddings", "masks", "labels")]

    def run(tag, extra):
        out = tmp_path / tag
        y = dict(encoder_configs=cfg["encoder_configs"], modality_config=mod_cfg, hidden_size=cfg["dim"], layers=cfg["depth"], heads=cfg["heads"],
                 dim_head=cfg["dim_head"], num_fusion_tokens=cfg["num_fusion_tokens"], batch_size=4, fcl=cfg["fcl"], fcl_root=cfg["fcl_root"],
                 bimodal_contrastive=cfg["bimodal_contrastive"], non_fusion_fcl=cfg["non_fusion_fcl"], fusion_combos=cfg["fusion_combos"],
                 zorro=cfg["zorro"], output_dir=str(out), dataset="unused", label_col="Labels")
        ypath = tmp_path / f"{tag}.yaml"
        ypath.write_text(yaml.safe_dump(y, sort_keys=False))
        r = subprocess.run([sys.executable, os.path.join(REPO, "infer_accel_gpu.py"), str(ypath), "--synthetic", "2"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return out, ypath

    plain, _ = run("plain", [])
    ro_dir, ypath = run("readout", ["--readout"])
    listing = lambda d: sorted(f for f in os.listdir(d) if f.endswith(".pt"))          # (beside the config copy the loader leaves there)
    assert listing(plain) == sorted(old)
    assert listing(ro_dir) == sorted(old + ["train_attention.pt", "eval_attention.pt"])
    for f in old:
        assert open(plain / f, "rb").read() == open(ro_dir / f, "rb").read(), f
    # the method on the script's model (same seed) and batches
    config = P.config.training_config(str(ypath))
    torch.manual_seed(0)
    model_config = P.config.get_model_config(config)
    model = P.build_model(model_config).to(DEV).eval()
    RO = importlib.import_module("mca-paper_amd.readout")
    for tv, seed0 in (("train", 100), ("eval", 10_000)):
        att = torch.load(ro_dir / f"{tv}_attention.pt", weights_only=False)
        assert set(att) == {"groups", "slot_mass"} and att["groups"] == RO.group_names(model)
        assert set(att["slot_mass"]) == set(model.output_slots())
        want = {k: [] for k in model.output_slots()}
        for i in range(2):
            bt = to_device(P.data.synthetic_batch(model_config, config.batch_size, seed=seed0 + i, p_drop=0.2), DEV)
            for k, v in model.attention_readout(bt, layers=[], pool=True)["slot_mass"].items():
                want[k].append(v.cpu())
        for k, v in att["slot_mass"].items():
            assert v.shape == (8, len(att["groups"])) and torch.equal(v, torch.cat(want[k], 0)), k
