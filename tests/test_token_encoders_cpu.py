"""SequenceEncoder and SparseTabularEncoder, host side (no GPU): registration, the reference's module tree and same-seed weights
(tests/golden/token_encoders_tiny.pt, written by tools/make_token_encoder_goldens.py from the reference's own classes), the
synthetic batches, and the deterministic-scratch bookkeeping of their step objects."""
import copy
import importlib
import math
import os
import types

import pytest
import torch

from util_small import GOLDEN, small_config

TYPES = ("SequenceEncoder", "SparseTabularEncoder")


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLDEN, "token_encoders_tiny.pt"), weights_only=False)


def token_config(variant):
    """small_config with text as a SequenceEncoder and (MCA only) video as a SparseTabularEncoder"""
    cfg = small_config(variant)
    enc = cfg["encoder_configs"]
    enc["text"] = {"type": "SequenceEncoder", "num_embeddings": 37, "max_tokens": 30, "embedding_dim": 128}
    if variant == "mca":
        enc["video"] = {"type": "SparseTabularEncoder", "num_embeddings": 23, "max_tokens": 45, "max_value": 100, "embedding_dim": 128}
    return cfg


def test_registered_and_models_construct(pkg):
    encs = importlib.import_module("mca-paper_amd.encoders")
    for t in TYPES:
        assert issubclass(pkg.encoders_dict[t], encs.NativeEncoder)
    kinds = {pkg.encoders_dict[t].kind for t in TYPES} | {encs.EmbeddedSequenceEncoder.kind, encs.TabularEncoder.kind}
    assert len(kinds) == 4 and "" not in kinds
    m = pkg.build_model(token_config("mca"))
    assert type(m).__name__ == "MCA" and isinstance(m.encoders["text"], encs.SequenceEncoder)
    assert isinstance(m.encoders["video"], encs.SparseTabularEncoder)
    assert m.structure.token_dims == [70, 45, 30] or list(m.structure.token_dims) == [70, 45, 30]
    e = pkg.build_model(token_config("eao"))
    assert type(e).__name__ == "EAO" and isinstance(e.encoders["text"], encs.SequenceEncoder)
    # the num_embeddings == max_tokens rule is the dense TabularEncoder's alone
    bad = small_config("tab")
    bad["encoder_configs"]["video"]["num_embeddings"] = 44
    with pytest.raises(ValueError, match="num_embeddings"):
        pkg.build_model(bad)
    import encoders as shim
    assert shim.SequenceEncoder is encs.SequenceEncoder and shim.SparseTabularEncoder is encs.SparseTabularEncoder


@pytest.mark.parametrize("t", TYPES)
def test_state_dict_keys_and_same_seed_init_as_reference(pkg, gold, t):
    rec = gold[t]
    torch.manual_seed(rec["seed"])
    enc = pkg.encoders_dict[t](**copy.deepcopy(rec["config"]))
    sd = enc.state_dict()
    assert list(sd.keys()) == list(rec["init"].keys())
    for k, want in rec["init"].items():
        v = sd[k]
        assert v.shape == want.shape and v.dtype == want.dtype, k
        if k.endswith("positional_encoder.pe"):
            # the sinusoidal table takes no seed and its float32 exp / sin / cos differ in the last bit between hosts: every element is
            # the formula in fp64 within the float32 rounding of its frequency and angle plus one ulp (tests/test_host_cpu.py)
            L, d = v.shape
            freq = torch.exp(torch.arange(0, d, 2, dtype=torch.float64) * (-math.log(10000.0) / d))
            ang = torch.arange(L, dtype=torch.float64).unsqueeze(1) * freq
            ideal = torch.stack([torch.sin(ang), torch.cos(ang)], -1).reshape(L, d)
            bound = torch.repeat_interleave(ang, 2, dim=1) * 2.0 ** -21 + 2.0 ** -22
            assert bool(((v.double() - ideal).abs() <= bound).all()) and bool(((want.double() - ideal).abs() <= bound).all()), k
        else:
            assert torch.equal(v, want), k
    pad = enc.token_encoder.embedding.padding_idx
    assert pad == 0 and float(sd["token_encoder.embedding.weight"][pad].abs().sum()) == 0.0
    assert "index" not in sd


@pytest.mark.parametrize("t", TYPES)
def test_native_encoder_forward_still_raises(pkg, gold, t):
    enc = pkg.encoders_dict[t](**copy.deepcopy(gold[t]["config"]))
    with pytest.raises(NotImplementedError, match="parameter container"):
        enc(gold[t]["batch"])


def test_synthetic_batch_keys_and_dtypes(pkg):
    cfg = token_config("mca")
    b = 6
    batch = pkg.data.synthetic_batch(cfg, b, seed=3, p_drop=0.4)
    text, video = batch["text"], batch["video"]
    assert set(text) == {"tokens", "attention_mask"} and set(video) == {"indices", "data", "attention_mask"}
    for idx, V, n, m in ((text["tokens"], 37, 30, text), (video["indices"], 23, 45, video)):
        assert idx.dtype == torch.int64 and idx.shape == (b, n)
        assert m["attention_mask"].dtype == torch.int64 and torch.equal(m["attention_mask"], (idx == 0).to(torch.int64))
        assert int(idx.min()) >= 0 and int(idx.max()) < V
        valid = (idx != 0).sum(1)
        for s in range(b):          # pad token 0 past the valid length only
            assert bool((idx[s, :valid[s]] != 0).all()) and bool((idx[s, valid[s]:] == 0).all())
    assert video["data"].dtype == torch.float32 and video["data"].shape == (b, 45)
    assert bool(((video["data"] == 0.0) == (video["indices"] == 0)).all())
    dropped = [(batch[k]["attention_mask"] != 0).all(1) for k in ("text", "video")]
    assert bool(dropped[0].any() or dropped[1].any())          # p_drop = 0.4 over 12 draws with this seed drops some
    assert "tokens" in pkg.data.synthetic_batch(cfg, 2, lengths="full")["text"]


def test_det_shapes_feed_det_need_without_gpu(pkg):
    """the step objects of the new kinds, built against a stand-in engine on the CPU: their det_shapes() name the table gradient,
    and FusionEngine._det_need turns it into the library's size query"""
    steps = importlib.import_module("mca-paper_amd.encoder_steps")
    engine = importlib.import_module("mca-paper_amd.engine")
    L = importlib.import_module("mca-paper_amd.hip").lib()
    m = pkg.build_model(token_config("mca"))
    D, b = 128, 4
    eng = types.SimpleNamespace(st=m.structure, offsets=[0, 70, 115, 145], D=D, N=153, grad_of=lambda p: None, device="cpu",
                                I=int(D * 4 * 2 / 3), R=m.structure.n_return, F=8)
    eng.enc_steps = [steps.step_for(eng, name, mi, m.encoders[name]) for mi, name in enumerate(m.modality_types)]
    assert [type(s).__name__ for s in eng.enc_steps] == ["SequenceStep", "SparseTabularStep", "TokenSequenceStep"]
    assert all(s.native for s in eng.enc_steps)
    seq, sparse = eng.enc_steps[2], eng.enc_steps[1]
    assert seq.det_shapes(b) == dict(emb=[b * 30])
    assert sparse.det_shapes(b) == dict(emb=[b * 45], ln=[(b * 45, D)], tn=[(b * 45, D, D)], tab=[b * 45])
    assert seq.marker.dtype == torch.int32 and seq.marker.shape == (37,) and int(seq.marker.abs().sum()) == 0
    assert L.mca_embedding_scatter_add_det_scratch(600) == 1200 and L.mca_embedding_scatter_add_det_scratch(0) == 0
    need = engine.FusionEngine._det_need(eng, b)
    assert need >= L.mca_embedding_scatter_add_det_scratch(b * 45)
    # a table gradient larger than every other launch of the step decides the figure
    seq.det_shapes = lambda b: dict(emb=[10 ** 9])
    assert engine.FusionEngine._det_need(eng, b) == 2 * 10 ** 9


def test_flag_inputs_skips_integer_tensors(pkg):
    engine = importlib.import_module("mca-paper_amd.engine")
    seen = []
    eng = types.SimpleNamespace(_flag_tensors=lambda ts, bit: seen.append((ts, bit)))
    batch = pkg.data.synthetic_batch(token_config("mca"), 2, seed=1)
    engine.FusionEngine._flag_inputs(eng, batch)
    (ts, bit), = seen
    assert bit == 1 and len(ts) == 1 and ts[0] is batch["audio"]["tokens"]          # not the int64 `tokens` of text
