"""PatchEncoder, host side (no GPU): registration, the reference's module tree and same-seed weights (tests/golden/patch_encoder_tiny.pt,
written by tools/make_patch_encoder_goldens.py from the reference's own class), the torch twin the GPU tests measure against held
to that fixture, every refusal, the synthetic batch and the collator, the step object's deterministic-scratch bookkeeping, and the
kernel test's drivers and data (tests/patch_cases.py) on an fp32 restatement of the kernel."""
import copy
import ctypes
import importlib
import os
import types

import pytest
import torch

import patch_cases as pc
from patch_twin import TWIN, TwinPatchEncoder, patch_config, patches
from util_small import GOLDEN, rel_err, small_config


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLDEN, "patch_encoder_tiny.pt"), weights_only=False)


def test_registered_and_models_construct(pkg):
    encs = importlib.import_module("mca-paper_amd.encoders")
    cls = pkg.encoders_dict["PatchEncoder"]
    assert issubclass(cls, encs.NativeEncoder)
    kinds = {c.kind for c in (cls, encs.EmbeddedSequenceEncoder, encs.TabularEncoder, encs.SequenceEncoder, encs.SparseTabularEncoder)}
    assert len(kinds) == 5 and "" not in kinds
    from encoders import PatchEncoder
    import encoders as shim
    assert PatchEncoder is cls and "PatchEncoder" in shim.__all__
    m = pkg.build_model(patch_config(small_config, "mca"))
    assert type(m).__name__ == "MCA" and isinstance(m.encoders["audio"], cls) and list(m.structure.token_dims) == [70, 45, 30]
    e = pkg.build_model(patch_config(small_config, "eao"))
    assert type(e).__name__ == "EAO" and isinstance(e.encoders["audio"], cls)
    enc = m.encoders["audio"]
    assert (enc.embedding_dim, enc.max_tokens, tuple(enc.patch_size), enc.pad_token) == (128, 70, (4, 5), -10000)
    assert cls(pad_token=7, dropout=0.0).pad_token == -10000          # the reference overwrites the argument (encoders.py:239)
    assert "einops" not in open(encs.__file__).read()


@pytest.mark.parametrize("i", [0, 1])
def test_state_dict_keys_and_same_seed_init_as_reference(pkg, gold, i):
    rec = gold["configs"][i]
    torch.manual_seed(rec["seed"])
    enc = pkg.encoders_dict["PatchEncoder"](**copy.deepcopy(rec["config"]))
    sd = enc.state_dict()
    assert list(sd.keys()) == list(rec["init"].keys())
    assert {"batch_to_tokens.1.weight", "batch_to_tokens.2.bias", "batch_to_tokens.3.weight", "index", "embedding.weight"} <= set(sd)
    for k, want in rec["init"].items():
        assert sd[k].shape == want.shape and sd[k].dtype == want.dtype and torch.equal(sd[k], want), k
    with pytest.raises(NotImplementedError, match="parameter container"):
        enc(rec["batch"])


@pytest.mark.parametrize("i", [0, 1])
def test_twin_reproduces_the_reference_fixture(gold, i):
    """torch against torch in fp32: 1e-5 rel-L2 on tokens (mask 0) and every gradient; a larger gap would be a restatement error.
    Tokens of all-pad patches at 1e-3 absolute only: LayerNorm of a constant row is ill-conditioned in torch itself."""
    rec = gold["configs"][i]
    twin = TwinPatchEncoder(**copy.deepcopy(rec["config"]))
    assert list(twin.state_dict().keys()) == list(rec["weights"].keys())
    twin.load_state_dict(rec["weights"])
    tokens, mask = twin(rec["batch"])
    assert mask.dtype == torch.int64 and torch.equal(mask, rec["mask"])
    live = rec["mask"] == 0
    assert 0 < int(live.sum()) < live.numel()
    assert rel_err(tokens[live], rec["tokens"][live]) <= 1e-5
    assert float((tokens.detach()[~live] - rec["tokens"][~live]).abs().max()) <= 1e-3
    tokens.retain_grad()
    tokens[mask == 0].square().sum().backward()
    assert rel_err(tokens.grad, rec["upstream"]) <= 1e-5
    grads = dict(twin.named_parameters())
    assert set(grads) == set(rec["grads"])
    for k, want in rec["grads"].items():
        assert float(want.abs().max()) > 0 and rel_err(grads[k].grad, want) <= 1e-5, k
    # the fixture's batch has what its docstring says: partly padded patches that are not masked, and a lone pad value
    x = patches(rec["batch"]["values"], *rec["config"]["patch_size"])
    some, every = (x == -10000).any(-1), (x == -10000).all(-1)
    assert bool((some & ~every)[0].any()) and bool(every[1].all()) and int((some & ~every)[2].sum()) == 1


def test_refusals(pkg, gold):
    cls = pkg.encoders_dict["PatchEncoder"]
    ok = dict(patch_size=[4, 5], max_tokens=70, embedding_dim=128, dropout=0.0)
    cls(**ok)
    for mode in ("image", "video"):
        with pytest.raises(NotImplementedError, match=mode):
            cls(**dict(ok, mode=mode, num_channels=3, patch_size=[2, 2] if mode == "image" else [2, 2, 2]))
        r = gold["unrunnable"][mode]
        assert r["class"] and r["text"] and r["stage"] in ("construct", "call")          # the reference cannot run it either
    with pytest.raises(NotImplementedError, match="attn_mask"):
        cls(**dict(ok, attn_mask=False))
    with pytest.raises(NotImplementedError, match="dropout: 0.0"):
        cls(**dict(ok, dropout=0.1))
    with pytest.raises(NotImplementedError, match="dropout"):
        cls(patch_size=[4, 5], max_tokens=70, embedding_dim=128)          # the reference's default is 0.1
    with pytest.raises(NotImplementedError, match="1024"):
        cls(**dict(ok, patch_size=[33, 32]))
    cls(**dict(ok, patch_size=[32, 32]))
    cls(**dict(ok, input_shape=[40, 35]))
    for shape in ([40, 30], [41, 35], [40, 36]):
        with pytest.raises(ValueError, match="input_shape"):
            cls(**dict(ok, input_shape=shape))
    bad = patch_config(small_config, "mca")
    bad["encoder_configs"]["audio"]["dropout"] = 0.1
    with pytest.raises(NotImplementedError, match="dropout"):
        pkg.build_model(bad)


def test_synthetic_batch(pkg):
    cfg = patch_config(small_config, "mca")
    b = 8
    batch = pkg.data.synthetic_batch(cfg, b, seed=3, p_drop=0.4, lengths="uniform")
    assert set(batch["audio"]) == {"values"}
    v = batch["audio"]["values"]
    assert v.shape == (b, 40, 35) and v.dtype == torch.float32
    x = patches(v, 4, 5)
    some, every = (x == -10000).any(-1), (x == -10000).all(-1)
    dropped = every.all(1)
    assert bool(dropped.any()) and not bool(dropped.all())          # p_drop = 0.4 over 8 samples with this seed
    assert bool((v[dropped] == -10000).all())
    assert bool((some & ~every).any()), "no partly padded patch: a valid row count inside a patch row"
    rows_pad = (v == -10000).all(2)
    for s in range(b):          # -10000 past the valid row count only
        k = int((~rows_pad[s]).sum())
        assert bool((~rows_pad[s, :k]).all()) and bool(rows_pad[s, k:].all())
    full = pkg.data.synthetic_batch(cfg, 2, lengths="full")["audio"]["values"]
    assert not bool((full == -10000).any())
    del cfg["encoder_configs"]["audio"]["input_shape"]
    with pytest.raises(ValueError, match="input_shape"):
        pkg.data.synthetic_batch(cfg, 2)


def test_matrix_collator_feeds_the_step_shape(pkg):
    coll = pkg.MultimodalCollator({"audio": {"type": "matrix", "pad_len": 40, "max_channels": 35}})
    g = torch.Generator().manual_seed(1)
    out = coll([{"audio": {"values": torch.randn(17, 35, generator=g)}}, {"audio": {"values": None}},
                {"audio": {"values": torch.randn(50, 35, generator=g)}}])
    v = out["audio"]["values"]
    assert v.shape == (3, 40, 35) and v.dtype == torch.float32 and "attention_mask" not in out["audio"]
    assert bool((v[1] == -10000).all()) and bool((v[0, 17:] == -10000).all()) and not bool((v[0, :17] == -10000).any())
    every = (patches(v, 4, 5) == -10000).all(-1)
    assert bool(every[1].all()) and int(every[0].sum()) == 5 * 7 and not bool(every[2].any())          # rows 17 .. 19 cut patch row 4


def test_step_object_and_det_shapes_without_gpu(pkg):
    steps = importlib.import_module("mca-paper_amd.encoder_steps")
    engine = importlib.import_module("mca-paper_amd.engine")
    L = importlib.import_module("mca-paper_amd.hip").lib()
    m = pkg.build_model(patch_config(small_config, "mca"))
    D, b = 128, 4
    eng = types.SimpleNamespace(st=m.structure, offsets=[0, 70, 115, 145], D=D, N=153, grad_of=lambda p: None, device="cpu",
                                I=int(D * 4 * 2 / 3), R=m.structure.n_return, F=8)
    eng.enc_steps = [steps.step_for(eng, name, mi, m.encoders[name]) for mi, name in enumerate(m.modality_types)]
    assert [type(s).__name__ for s in eng.enc_steps] == ["PatchStep", "SequenceStep", "SequenceStep"]
    st = eng.enc_steps[0]
    assert st.native and (st.P, st.kp) == (20, 64) and st.w.shape == (D, 64) and st.wT.shape == (64, D)
    assert st.det_shapes(b) == dict(ln=[(280, D), (280, 20)], tn=[(280, D, 20)], rr=[(280, 70)])
    assert st.row_mask({}) is None
    # the hook the engine calls: the batch's own mask for every other step
    am = torch.zeros(b, 45, dtype=torch.bool)
    assert eng.enc_steps[1].attention_mask({"attention_mask": am}, {}) is am
    ws = engine.FusionEngine._det_need(eng, b)
    assert ws >= L.mca_layernorm_bwd_det_scratch(280, 20) and ws >= L.mca_reduce_rows_det_scratch(280, 70, D)
    # values of another shape are refused before any launch (no library call can be reached on this CPU tensor)
    fake_ws = {"b": b, "enc": {"audio": {}}}
    with pytest.raises(AssertionError, match="60 - 70"):
        st.attention_mask({"values": torch.zeros(b, 40, 30)}, fake_ws)
    with pytest.raises(AssertionError, match="whole number"):
        st.attention_mask({"values": torch.zeros(b, 41, 35)}, fake_ws)
    assert "values" not in fake_ws["enc"]["audio"]


def test_library_exports_the_kernel_and_refuses_bad_shapes_on_the_host(pkg):
    """the refusals are host-side checks that launch nothing: they answer without a GPU"""
    hip = importlib.import_module("mca-paper_amd.hip")
    L = hip.lib()
    assert hasattr(L, "mca_patch_ln_fwd")
    one = ctypes.c_void_p(64)          # never dereferenced: every call below is refused before a launch
    def rc(H=8, W=8, p1=4, p2=4, cols_pad=64, values=one, ld=64):
        return L.mca_patch_ln_fwd(values, H * W, W, 2, H, W, p1, p2, one, one, -10000.0, 1e-5, None, one, ld, cols_pad, one, one, one, None)
    assert rc(H=9) != 0 and rc(W=9) != 0 and rc(H=66, W=64, p1=33, p2=32, cols_pad=1088, ld=1088) != 0
    assert rc(cols_pad=15) != 0 and rc(values=None) != 0 and rc(ld=32) != 0


@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_kernel_drivers_and_data_on_the_fp32_restatement(c):
    """what tests/test_patch_encoder_gpu.py does to the kernel, done to its restatement: the drivers work, every bound is
    satisfiable, the plain data keeps the precondition's cap, and over the variants every row is of every kind"""
    gen = torch.Generator().manual_seed(5)
    T, O = pc.setup(c, pc.plain_rows(c, gen), gen)
    pc.emulate_into(T, O)
    live, skipped = pc.check(T, O, pc.case_id(c) + " plain", cap=pc.MAX_EXCLUDED)
    assert live > 0 and skipped == 0
    seen = torch.zeros(T["rows"], pc.N_KINDS, dtype=torch.bool)
    checked = 0
    for v in range(pc.N_KINDS):
        rows = pc.special_rows(c, v, gen)
        T, O = pc.setup(c, rows, gen, ldv_extra=4, with_xp=v % 2 == 0)
        pc.emulate_into(T, O)
        live, skipped = pc.check(T, O, f"{pc.case_id(c)} special {v}")
        checked += live - skipped
        seen[torch.arange(T["rows"]), (torch.arange(T["rows"]) + v) % pc.N_KINDS] = True
    assert bool(seen.all()) and checked > 0
