"""ImagePatchEncoder / VideoPatchEncoder, host side (no GPU): registration, the reference's module tree and same-seed weights
(tests/golden/patch_encoder_nd_tiny.pt, written by tools/make_patch_nd_goldens.py from the reference's own class in modes "image" and
"video"), the torch twins the GPU tests measure against held to that fixture, every refusal, the collators, the synthetic batch, the
step object's bookkeeping, the C ABI's argument refusals, and the kernel test's drivers and data (tests/patch_nd_cases.py) on an fp32
restatement of the kernel."""
import copy
import ctypes
import importlib
import os
import types

import pytest
import torch

import patch_cases as pc
import patch_nd_cases as nd
from patch_nd_twin import ND_CFG, TWIN_CLASSES, TWINS, nd_config, patches_nd, reference_tokens
from util_small import GOLDEN, rel_err, small_config

MODES = {"image": "ImagePatchEncoder", "video": "VideoPatchEncoder"}


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLDEN, "patch_encoder_nd_tiny.pt"), weights_only=False)


def test_fixture_is_small(gold):
    """same-seed weights, gradients and `batch_to_tokens` output of two encoders at D = 128: about 170 KB, a sixth of the limit for a
    committed file; nothing in it is stored twice"""
    assert os.path.getsize(os.path.join(GOLDEN, "patch_encoder_nd_tiny.pt")) < 192 * 1024
    for rec in gold.values():
        assert set(rec) == {"config", "seed", "init", "ln", "batch", "rearranged", "pre", "mask", "grads"}


def test_registered_and_models_construct(pkg):
    encs = importlib.import_module("mca-paper_amd.encoders")
    import encoders as shim
    native = [c for c in pkg.encoders_dict.values() if issubclass(c, encs.NativeEncoder)]
    kinds = {c.kind for c in native}
    assert len(kinds) == len(native) == 7 and "" not in kinds
    for mode, name in MODES.items():
        cls = pkg.encoders_dict[name]
        assert issubclass(cls, encs.NativeEncoder) and cls.kind == mode + "_patch"
        assert getattr(shim, name) is cls and name in shim.__all__
        for variant, model in (("mca", "MCA"), ("eao", "EAO")):
            m = pkg.build_model(nd_config(small_config, variant, mode))
            assert type(m).__name__ == model and isinstance(m.encoders["audio"], cls)
            assert list(m.structure.token_dims) == [ND_CFG[mode]["max_tokens"], 45, 30]
        enc = m.encoders["audio"]
        assert (enc.embedding_dim, enc.pad_token, tuple(enc.patch_size)) == (128, -10000, tuple(ND_CFG[mode]["patch_size"]))
        assert cls(**dict(ND_CFG[mode], pad_token=7)).pad_token == -10000          # the reference overwrites the argument (encoders.py:239)
    assert "einops" not in open(encs.__file__).read()


@pytest.mark.parametrize("mode", list(MODES))
def test_state_dict_keys_and_same_seed_init_as_reference(pkg, gold, mode):
    rec = gold[mode]
    assert rec["config"]["type"] == MODES[mode]
    torch.manual_seed(rec["seed"])
    enc = pkg.encoders_dict[MODES[mode]](**copy.deepcopy(rec["config"]))
    sd = enc.state_dict()
    assert list(sd.keys()) == list(rec["init"].keys())
    assert {"batch_to_tokens.1.weight", "batch_to_tokens.2.bias", "batch_to_tokens.3.weight", "index", "embedding.weight"} <= set(sd)
    for k, want in rec["init"].items():
        assert sd[k].shape == want.shape and sd[k].dtype == want.dtype and torch.equal(sd[k], want), k
    with pytest.raises(NotImplementedError, match="parameter container"):
        enc(rec["batch"])


@pytest.mark.parametrize("mode", list(MODES))
def test_twin_reproduces_the_reference_fixture(gold, mode):
    """torch against torch in fp32, the bounds of test_patch_encoder_cpu.py::test_twin_reproduces_the_reference_fixture: the
    rearrangement bit-equal, the mask equal, tokens (mask 0) and every gradient 1e-5 rel-L2, tokens of all-pad patches 1e-3 absolute"""
    rec = gold[mode]
    cfg = rec["config"]
    twin = TWIN_CLASSES[TWINS[MODES[mode]]](**copy.deepcopy(cfg))
    weights = dict(rec["init"], **rec["ln"])
    assert list(twin.state_dict().keys()) == list(rec["init"].keys())
    twin.load_state_dict(weights)
    x = patches_nd(rec["batch"]["values"], cfg["patch_size"])
    assert x.shape == rec["rearranged"].shape and torch.equal(x.view(torch.int32), rec["rearranged"].view(torch.int32))
    tokens, mask = twin(rec["batch"])
    assert mask.dtype == torch.int64 and torch.equal(mask, rec["mask"])
    want, upstream = reference_tokens(rec)
    live = rec["mask"] == 0
    assert 0 < int(live.sum()) < live.numel()
    assert rel_err(tokens[live], want[live]) <= 1e-5
    assert float((tokens.detach()[~live] - want[~live]).abs().max()) <= 1e-3
    tokens.retain_grad()
    tokens[mask == 0].square().sum().backward()
    assert rel_err(tokens.grad, upstream) <= 1e-5
    grads = dict(twin.named_parameters())
    assert set(grads) == set(rec["grads"])
    for k, w in rec["grads"].items():
        assert float(w.abs().max()) > 0 and rel_err(grads[k].grad, w) <= 1e-5, k
    # the fixture's batch has what its docstring says
    C = cfg["num_channels"]
    xf = x.flatten(1, -2)
    some, every = (xf == -10000).any(-1), (xf == -10000).all(-1)
    per_channel = (xf.reshape(*xf.shape[:2], C, -1) == -10000).all(-1)          # (b, l, C): a whole channel of the patch is pad
    assert bool((per_channel.sum(-1) == 1)[0].any()), "no patch with a single all-pad channel"
    assert bool((some & ~every & (per_channel.sum(-1) == 0))[0].any()), "no partly padded patch"
    assert bool(every[0].any()) and bool(every[1].all()) and int((xf[2] == -10000).sum()) == 1


def test_refusals(pkg):
    for mode, name in MODES.items():
        cls = pkg.encoders_dict[name]
        ok = copy.deepcopy(ND_CFG[mode])
        cls(**ok)
        with pytest.raises(AssertionError):
            cls(**dict(ok, patch_size=ok["patch_size"] + [2]))
        with pytest.raises(ValueError, match="num_channels"):
            cls(**dict(ok, num_channels=0))
        noc = dict(ok)
        del noc["num_channels"]
        with pytest.raises(ValueError, match="num_channels"):
            cls(**noc)                                                 # the reference's default
        with pytest.raises(NotImplementedError, match="attn_mask"):
            cls(**dict(ok, attn_mask=False))
        with pytest.raises(NotImplementedError, match="dropout: 0.0"):
            cls(**dict(ok, dropout=0.1))
        nod = dict(ok)
        del nod["dropout"]
        with pytest.raises(NotImplementedError, match="dropout"):
            cls(**nod)                                                 # the reference's default is 0.1
        big = [16, 16] if mode == "image" else [2, 8, 16]
        cls(**dict(ok, patch_size=big, num_channels=4, input_shape=None))          # P = 1024
        with pytest.raises(NotImplementedError, match=r"(?s)5 channels.*1024"):
            cls(**dict(ok, patch_size=big, num_channels=5, input_shape=None))
        shape = ok["input_shape"]
        for i in range(len(shape)):
            for delta in (1, ok["patch_size"][i]):          # not divisible; divisible with another grid
                bad = list(shape)
                bad[i] += delta
                with pytest.raises(ValueError, match="input_shape"):
                    cls(**dict(ok, input_shape=bad))
        with pytest.raises(ValueError, match="input_shape"):
            cls(**dict(ok, input_shape=shape + [4]))
        bad = nd_config(small_config, "mca", mode)
        bad["encoder_configs"]["audio"]["dropout"] = 0.1
        with pytest.raises(NotImplementedError, match="dropout"):
            pkg.build_model(bad)
    # PatchEncoder's own modes stay refused
    for mode in MODES:
        with pytest.raises(NotImplementedError, match=mode):
            pkg.encoders_dict["PatchEncoder"](mode=mode, num_channels=3, dropout=0.0, patch_size=[2, 2] if mode == "image" else [2, 2, 2])


# ------------------------------------------------------------------------------------------------ collators
def _image(g, shape=(3, 8, 15)):
    return torch.randn(*shape, generator=g)


def test_collators(pkg):
    assert {"image", "video"} <= set(pkg.collators)
    coll = pkg.MultimodalCollator({"pic": {"type": "image", "num_channels": 3, "input_shape": [8, 15]},
                                   "clip": {"type": "video", "num_channels": 2, "input_shape": [4, 8, 10]}})
    g = torch.Generator().manual_seed(1)
    pics = [_image(g), None, _image(g)]
    clips = [torch.randn(2, 4, 8, 10, generator=g), torch.randn(2, 2, 8, 10, generator=g), torch.randn(2, 7, 8, 10, generator=g)]
    out = coll([{"pic": {"values": p}, "clip": {"values": c}} for p, c in zip(pics, clips)])
    v, w = out["pic"]["values"], out["clip"]["values"]
    assert set(out["pic"]) == set(out["clip"]) == {"values"}
    assert v.shape == (3, 3, 8, 15) and v.dtype == torch.float32 and w.shape == (3, 2, 4, 8, 10) and w.dtype == torch.float32
    assert torch.equal(v[0], pics[0]) and torch.equal(v[2], pics[2]) and bool((v[1] == -10000).all())          # None: a block of pad
    assert torch.equal(w[0], clips[0])
    assert torch.equal(w[1, :, :2], clips[1]) and bool((w[1, :, 2:] == -10000).all())          # short clip: padded at the end
    assert torch.equal(w[2], clips[2][:, :4])                                                  # long clip: cropped
    every = (patches_nd(w, (2, 4, 5)) == -10000).all(-1).flatten(1)          # tokens (ti, hi, wi): temporal patch 1 of the short clip is masked
    assert not bool(every[0].any()) and not bool(every[2].any()) and every[1].tolist() == [False] * 4 + [True] * 4
    assert bool((patches_nd(v, (4, 5)) == -10000).all(-1)[1].all())
    one = pkg.MultimodalCollator({"clip": {"type": "video", "num_channels": 2, "input_shape": [4, 8, 10]}})
    assert bool((one([{"clip": {"values": None}}])["clip"]["values"] == -10000).all())
    for bad in (torch.zeros(3, 8, 14), torch.zeros(2, 8, 15), torch.zeros(3, 9, 15), torch.zeros(8, 15), torch.zeros(3, 1, 8, 15)):
        with pytest.raises(ValueError, match=r"\(3, 8, 15\)"):
            coll([{"pic": {"values": bad}, "clip": {"values": None}}])
    for bad in (torch.zeros(2, 4, 8, 9), torch.zeros(3, 4, 8, 10), torch.zeros(2, 4, 7, 10), torch.zeros(2, 8, 10)):
        with pytest.raises(ValueError, match=r"\(2, 4, 8, 10\)"):
            coll([{"pic": {"values": None}, "clip": {"values": bad}}])
    with pytest.raises(ValueError, match="input_shape"):
        pkg.MultimodalCollator({"pic": {"type": "image", "num_channels": 3, "input_shape": [4, 8, 15]}})


class _Samples(torch.utils.data.Dataset):
    def __len__(self):
        return 8

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(200 + i)
        return {"pic": {"values": None if i % 5 == 3 else _image(g)},
                "clip": {"values": torch.randn(2, int(torch.randint(1, 7, (1,), generator=g)), 8, 10, generator=g)}}


def test_collators_in_loader_workers_build_the_same_batch_in_shared_memory(pkg):
    """as tests/test_aux_cpu.py checks the other collators: inside a DataLoader worker the buffer is allocated in shared memory, and
    the values are those of the in-process call"""
    from torch.utils.data import DataLoader
    col = pkg.MultimodalCollator({"pic": {"type": "image", "num_channels": 3, "input_shape": [8, 15]},
                                  "clip": {"type": "video", "num_channels": 2, "input_shape": [4, 8, 10]}})
    ds = _Samples()
    here = list(DataLoader(ds, collate_fn=col, batch_size=4, num_workers=0))
    there = list(DataLoader(ds, collate_fn=col, batch_size=4, num_workers=2))
    assert len(here) == len(there) == 2
    for a, b in zip(here, there):
        for m in ("pic", "clip"):
            assert a[m]["values"].dtype == b[m]["values"].dtype and torch.equal(a[m]["values"], b[m]["values"])
            assert b[m]["values"].is_shared() and not a[m]["values"].is_shared()
    assert bool((here[0]["pic"]["values"][3] == -10000).all())


# ------------------------------------------------------------------------------------------------ synthetic batch
@pytest.mark.parametrize("mode", list(MODES))
def test_synthetic_batch(pkg, mode):
    cfg = nd_config(small_config, "mca", mode)
    c, b = ND_CFG[mode], 8
    batch = pkg.data.synthetic_batch(cfg, b, seed=3, p_drop=0.4, lengths="uniform")
    assert set(batch["audio"]) == {"values"}
    v = batch["audio"]["values"]
    assert v.shape == (b, c["num_channels"], *c["input_shape"]) and v.dtype == torch.float32
    x = patches_nd(v, c["patch_size"]).flatten(1, -2)
    some, every = (x == -10000).any(-1), (x == -10000).all(-1)
    dropped = every.all(1)
    assert bool(dropped.any()) and not bool(dropped.all())          # p_drop = 0.4 over 8 samples with this seed
    assert bool((v[dropped] == -10000).all())
    assert bool((some & ~every).any()), "no partly padded patch: a valid count inside a patch"
    # -10000 past the valid count only, along the rows of an image / the frames of a clip, the same in every channel
    tail = (v == -10000).movedim(2, 1).flatten(2)          # (b, L, the rest)
    assert bool((tail.all(2) == tail.any(2)).all())
    line = tail.all(2)
    for s in range(b):
        k = int((~line[s]).sum())
        assert bool((~line[s, :k]).all()) and bool(line[s, k:].all())
    full = pkg.data.synthetic_batch(cfg, 2, lengths="full")["audio"]["values"]
    assert not bool((full == -10000).any())
    for missing in (None, "absent"):          # (None is the encoder's own default)
        if missing is None:
            cfg["encoder_configs"]["audio"]["input_shape"] = None
        else:
            del cfg["encoder_configs"]["audio"]["input_shape"]
        with pytest.raises(ValueError, match="input_shape"):
            pkg.data.synthetic_batch(cfg, 2)


# ------------------------------------------------------------------------------------------------ the step object
@pytest.mark.parametrize("mode", list(MODES))
def test_step_object_and_det_shapes_without_gpu(pkg, mode):
    steps = importlib.import_module("mca-paper_amd.encoder_steps")
    engine = importlib.import_module("mca-paper_amd.engine")
    L = importlib.import_module("mca-paper_amd.hip").lib()
    m = pkg.build_model(nd_config(small_config, "mca", mode))
    c = ND_CFG[mode]
    n, D, b = c["max_tokens"], 128, 4
    P = c["num_channels"]
    for p in c["patch_size"]:
        P *= p
    eng = types.SimpleNamespace(st=m.structure, offsets=[0, n, n + 45, n + 75], D=D, N=n + 83, grad_of=lambda p: None, device="cpu",
                                I=int(D * 4 * 2 / 3), R=m.structure.n_return, F=8)
    eng.enc_steps = [steps.step_for(eng, name, mi, m.encoders[name]) for mi, name in enumerate(m.modality_types)]
    assert [type(s).__name__ for s in eng.enc_steps] == ["PatchNDStep", "SequenceStep", "SequenceStep"]
    st = eng.enc_steps[0]
    assert isinstance(st, steps.PatchStep) and st.native and type(st).forward is steps.PatchStep.forward and type(st).backward is steps.PatchStep.backward
    kp = (P + 63) // 64 * 64
    assert (st.P, st.kp) == (P, kp) and st.w.shape == (D, kp) and st.wT.shape == (kp, D)
    assert st.det_shapes(b) == dict(ln=[(b * n, D), (b * n, P)], tn=[(b * n, D, P)], rr=[(b * n, n)])
    assert st.row_mask({}) is None
    ws = engine.FusionEngine._det_need(eng, b)
    assert ws >= L.mca_layernorm_bwd_det_scratch(b * n, P) and ws >= L.mca_reduce_rows_det_scratch(b * n, n, D)
    # values of another shape are refused before any launch (no library call can be reached on these CPU tensors)
    fake_ws = {"b": b, "enc": {"audio": {}}}
    C, shape = c["num_channels"], c["input_shape"]
    wide = list(shape)
    wide[-1] += c["patch_size"][-1]
    grid = n // (shape[-1] // c["patch_size"][-1]) * (wide[-1] // c["patch_size"][-1])
    with pytest.raises(AssertionError, match=f"^{grid} - {n}$"):
        st.attention_mask({"values": torch.zeros(b, C, *wide)}, fake_ws)
    odd = list(shape)
    odd[0] += 1
    with pytest.raises(AssertionError, match="whole number"):
        st.attention_mask({"values": torch.zeros(b, C, *odd)}, fake_ws)
    for bad in (torch.zeros(b, C + 1, *shape), torch.zeros(b + 1, C, *shape), torch.zeros(b, *shape), torch.zeros(b, C, 1, *shape)):
        with pytest.raises(AssertionError, match="is not"):
            st.attention_mask({"values": bad}, fake_ws)
    assert "values" not in fake_ws["enc"]["audio"]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_the_kernel_and_refuses_bad_arguments_on_the_host(pkg):
    """the refusals are host-side checks that launch nothing: they answer without a GPU"""
    hip = importlib.import_module("mca-paper_amd.hip")
    L = hip.lib()
    assert hasattr(L, "mca_patch_nd_ln_fwd") and "mca_patch_nd_ln_fwd" in hip.SIGNATURES
    one = ctypes.c_void_p(64)          # never dereferenced: every call below is refused before a launch

    def rc(C=3, T=4, H=8, W=8, pt=2, p1=4, p2=4, cols_pad=128, ld=128, ldv=None, fs=None, cs=None, bs=None, batch=2, **ptrs):
        ldv = W if ldv is None else ldv
        fs = H * ldv if fs is None else fs
        cs = T * fs if cs is None else cs
        bs = C * cs if bs is None else bs
        p = dict(values=one, gamma=one, beta=one, xn=one, mean=one, rstd=one, mask=one)
        p.update(ptrs)
        return L.mca_patch_nd_ln_fwd(p["values"], bs, cs, fs, ldv, batch, C, T, H, W, pt, p1, p2, p["gamma"], p["beta"], -10000.0, 1e-5, None,
                                     p["xn"], ld, cols_pad, p["mean"], p["rstd"], p["mask"], None)
    assert rc(batch=0) == 0                                       # the same arguments are accepted (an empty batch launches nothing)
    assert rc(T=5) != 0 and rc(H=9) != 0 and rc(W=9) != 0, "T % pt, H % p1, W % p2"
    assert rc(C=0) != 0 and rc(pt=0) != 0 and rc(p1=0) != 0 and rc(p2=0) != 0 and rc(batch=-1) != 0
    assert rc(C=4, T=4, pt=4, H=16, p1=8, W=16, p2=8, cols_pad=1024, ld=1024, batch=0) == 0, "P = 1024"
    # P > 1024 alone: strides, cols_pad and ld_bf16 fit the dimensions and the batch is empty, so each call returns MCA_OK unless the
    # check on P fires; its neighbour with one dimension smaller (P <= 1024) is accepted
    over = dict(C=5, T=5, pt=5, H=41, p1=41, W=2, p2=1, cols_pad=1088, ld=1088, batch=0)
    assert rc(**over) == -1, "P = 5 * 5 * 41 * 1 = 1025"
    assert rc(**dict(over, H=40, p1=40)) == 0, "P = 1000"
    twice = dict(C=8, T=2, pt=2, H=16, p1=16, W=16, p2=8, cols_pad=2048, ld=2048, batch=0)
    assert rc(**twice) == -1, "P = 8 * 2 * 16 * 8 = 2048 (its span would still fit the LDS budget)"
    assert rc(**dict(twice, C=4)) == 0, "P = 1024"
    assert rc(C=1 << 20, T=1 << 10, pt=1 << 10, H=2, p1=2, W=2, p2=2) != 0, "a product that leaves 32 bits"
    assert rc(cols_pad=95) != 0 and rc(ld=64) != 0 and rc(ldv=7) != 0
    assert rc(fs=8 * 7 + 7) != 0 and rc(fs=8 * 7 + 8, cs=4 * 64, bs=3 * 4 * 64, batch=0) == 0, "frame stride below (H - 1) ldv + W"
    assert rc(cs=3 * 64 + 63) != 0 and rc(bs=2 * 256 + 255) != 0, "channel / batch stride below what it steps over"
    assert rc(T=1, pt=1, fs=0, cs=64, cols_pad=64, batch=0) == 0, "an image: the frame stride is not used"
    for k in ("values", "gamma", "beta", "xn", "mean", "rstd", "mask"):
        assert rc(**{k: None}) != 0, k


# ------------------------------------------------------------------------------------------------ the kernel test's drivers
def test_kinds_rotate_and_the_new_kind_is_checkable():
    c = nd.CASES[0]
    d = nd.dims(c)
    gen = torch.Generator().manual_seed(1)
    x = nd.special_rows(c, nd.N_KINDS - 1, gen)          # row 0 is of the new kind
    per_channel = (x[0].view(d["C"], -1) == nd.PAD).all(1)
    assert per_channel.tolist() == [True, False, False]
    pad, ok = pc.checkable(x[:1])
    assert not bool(pad[0]) and bool(ok[0])          # not masked; |mean| <= 4 std: its statistics are checked


@pytest.mark.parametrize("c", nd.CASES + nd.DEGENERATE, ids=nd.case_id)
def test_kernel_drivers_and_data_on_the_fp32_restatement(c):
    """what tests/test_patch_nd_gpu.py does to the kernel, done to its restatement (the gather through the four strides of the framed
    buffer, then patch_cases' fp32 formula): the drivers work, every bound is satisfiable, the plain data excludes no row from the
    statistics check (cap patch_cases.MAX_EXCLUDED asserted too), and over the variants every row is of every kind"""
    gen = torch.Generator().manual_seed(5)
    checked = 0
    for extra in (3, 4):
        T, O = nd.setup(c, nd.plain_rows(c, gen), gen, ldv_extra=extra)
        got = nd.gather_restated(T)
        assert torch.equal(got.view(torch.int32), T["x"].view(torch.int32))
        pc.emulate_into(dict(T, x=got), O)
        live, skipped = pc.check(T, O, nd.case_id(c) + " plain", cap=pc.MAX_EXCLUDED)
        assert live > 0 and skipped == 0
    seen = torch.zeros(T["rows"], nd.N_KINDS, dtype=torch.bool)
    for v in range(nd.N_KINDS):
        T, O = nd.setup(c, nd.special_rows(c, v, gen), gen, ldv_extra=3 + v % 2, with_xp=v % 2 == 0)
        pc.emulate_into(dict(T, x=nd.gather_restated(T)), O)
        live, skipped = pc.check(T, O, f"{nd.case_id(c)} special {v}")
        checked += live - skipped
        seen[torch.arange(T["rows"]), (torch.arange(T["rows"]) + v) % nd.N_KINDS] = True
    assert bool(seen.all()) and checked > 0
