"""CPU-side tests of the attention readout (readout.py, MCA.attention_readout): group names, the uniform-row shares, the
slot reduction, the refusals and the binding."""
import ctypes as C
import importlib
import types

import numpy as np
import pytest
import torch

from util_small import small_config


@pytest.fixture(scope="module")
def RO():
    return importlib.import_module("mca-paper_amd.readout")


@pytest.mark.parametrize("variant", ["mca", "zorro", "bimodal"])
def test_group_names_small(pkg, RO, variant):
    cfg = small_config(variant)
    m = pkg.build_model(cfg)
    names = RO.group_names(m)
    st = m.structure
    assert len(names) == st.n_groups == int(st.kgroup.max()) + 1
    assert names[:3] == ["audio", "video", "text"]
    if variant == "zorro":
        assert names[3:] == ["fusion"]
    else:          # fusion_combos [3, 2] of three modalities: {0,1,2}, {0,1}, {0,2}, {1,2}
        assert names[3:] == [frozenset({0, 1, 2}), frozenset({0, 1}), frozenset({0, 2}), frozenset({1, 2})]
        # the ids are the structure's: fusion sub-block c is key group M + c and sees the modalities of its combination
        off = sum(st.token_dims)
        for c, combo in enumerate(names[3:]):
            rows = np.nonzero(st.kgroup == 3 + c)[0]
            assert rows.min() == off + c * st.nsub and len(rows) == st.nsub
            assert int(st.qmask_attn[rows[0]]) == (1 << (3 + c)) | sum(1 << mi for mi in combo)
        # every fusion group is an output slot of the same name
        assert all(m.output_slots()[combo] == 3 + c for c, combo in enumerate(names[3:]))


def test_group_names_cmu(pkg, RO):
    m = pkg.MCA(**pkg.config.cmu_model_config(2))
    names = RO.group_names(m)
    assert len(names) == 15 == m.structure.n_groups
    assert names[:4] == list(m.modality_types)
    assert names[4] == frozenset({0, 1, 2, 3}) and [len(c) for c in names[4:]] == [4, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2]
    mz = pkg.MCA(**pkg.config.cmu_model_config(2, zorro=True))
    assert RO.group_names(mz) == list(mz.modality_types) + ["fusion"]


@pytest.mark.parametrize("dims,F,powers,zorro", [([70, 45, 30], 8, (3, 2), False), ([70, 45, 30], 8, (3, 2), True),
                                                 ([1500, 450, 450, 50], 88, (4, 3, 2), False), ([40, 30, 20, 10, 24], 32, (5, 4, 3), False)])
def test_uniform_mass_is_key_count_over_n(pkg, RO, dims, F, powers, zorro):
    st = pkg.structure.FusionStructure(dims, F, powers, fcl=not zorro, zorro=zorro)
    um = RO.uniform_mass(st)
    N = st.n_tokens
    assert um.dtype == np.float32 and um.shape == (st.n_groups,)
    for g in range(st.n_groups):
        assert um[g] == np.float32(int((st.kgroup == g).sum()) / N)
    assert um[:len(dims)].tolist() == [np.float32(d / N) for d in dims]
    assert abs(float(um.astype(np.float64).sum()) - 1.0) <= st.n_groups * 2.0 ** -24


def test_slot_mass_is_the_head_mean_of_the_slot_row(RO):
    rng = np.random.default_rng(0)
    pm = rng.random((3, 4, 5, 6)).astype(np.float32)          # (b, H, R, G)
    slots = {"a": 0, "b": 3, frozenset({0, 1}): 4, "fusion": 3}
    got = RO.slot_mass(torch.from_numpy(pm), slots)
    assert set(got) == set(slots)
    for k, row in slots.items():
        assert got[k].shape == (3, 6)
        np.testing.assert_allclose(got[k].numpy(), pm[:, :, row].astype(np.float64).mean(1), rtol=1e-6)


def test_eao_models_are_refused(pkg):
    m = pkg.build_model(small_config("eao"))
    with pytest.raises(NotImplementedError, match="EAO"):
        m.attention_readout({})


def test_fp8_attention_engine_is_refused(pkg):
    m = pkg.build_model(small_config("mca"))
    m._engine = types.SimpleNamespace(attn_dtype="fp8")          # (a real engine needs a GPU; the refusal comes before any launch)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.attention_readout({})


def test_binding_declares_the_entry_point_and_its_struct():
    hip = importlib.import_module("mca-paper_amd.hip")
    res, args = hip.SIGNATURES["mca_attn_readout"]
    assert res is C.c_int and args == [C.POINTER(hip.AttnReadoutArgs), C.c_void_p]
    names = [f[0] for f in hip.AttnReadoutArgs._fields_]
    assert names == ["q", "q_bstride", "q_ld", "k", "kv_bstride", "kv_ld", "lse", "qmask", "keyinfo", "ktile_flags", "q_ptr", "q_kt",
                     "q_order", "batch", "heads", "nq", "nk", "nk_pad", "n_qtiles", "n_ktiles", "scale", "flags", "n_groups",
                     "uniform_mass", "mass", "probs", "row0", "n_rows"]
    # the same layout as the C struct of include/mca_hip.h (LP64: 13 pointers / int64 + 9 x 4 bytes + 4 + pad, 3 pointers, 2 ints)
    assert C.sizeof(hip.AttnReadoutArgs) == 13 * 8 + 10 * 4 + 3 * 8 + 2 * 4
