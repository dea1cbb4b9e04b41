"""The case table and the checker of the attention edge tests, checked without a GPU: each case reaches the kernel paths it is
listed for (asserted from the schedules and a numpy restatement of the ktile_flags rule); an fp32 emulation that rounds where
the kernels round satisfies every derived bound with room to spare (the bounds are derived, not tuned, and satisfiable); and the
ways a kernel can be wrong on a few rows - an lse off by 0.05, a key tile left out, a dvmean forgotten, a row never stored, a
store outside the output - each make the checker raise and name the place."""
import re

import numpy as np
import pytest
import torch

import attention_cases as AC
import attention_edge_util as U
import gemm_edge_util as G

EMU_ELEMENT_MAX, EMU_ROW_MAX = 0.55, 0.30          # what the emulation must stay below (ROW_LIMIT = 0.5 is about twice its row ratio)


# ------------------------------------------------------------------------------------------- reach
def test_attention_edge_cases_reach_what_they_are_listed_for():
    # ---- aligned256, both variants
    for variant in ("mca", "zorro"):
        st, pad = AC.structure("aligned256", variant), AC.padding("aligned256")
        N = st.n_tokens
        assert N == 256 == AC.nk_pad_of(N) and int(st.kgroup.max()) <= 14
        fl = AC.ktile_flags(pad)
        assert fl.tolist() == [[0, 0, 2, 2], [2, 2, 0, 2], [2, 2, 2, 2], [1, 0, 1, 1], [0, 0, 0, 1]]
        sc = st.attn_schedule(128, 64)
        assert sc.q_kt[sc.q_ptr[0]:sc.q_ptr[1]].tolist() == [0, 1] and sc.q_full[sc.q_ptr[0]:sc.q_ptr[1]].tolist() == [1, 1]
        live = AC.dq_live_lists(st, pad)
        assert live[0, 0] == [] and live[4, 0] == []                                  # the dq pass: an empty live list
        assert live[2, 0] == [(0, True), (1, True)] and live[1, 0] == live[2, 0]      # the unmasked path ...
        assert len(live[2, 1]) == 4 and not any(u for _, u in live[2, 1])             # ... next to masked tiles of flag 2
        assert live[3, 0] == [(0, False)]                                             # the same structurally full tile, masked (flag 1)
        assert [t for t, _ in live[1, 1]] == [0, 1, 3]                                # key tile 2 dead inside a live list
        b128, b256 = AC.dkv_blocks(st, pad, 128), AC.dkv_blocks(st, pad, 256)
        assert b128[0, 0][0] and b128[0, 0][2] > 0 and not b128[0, 1][0]              # a dead 128-key block (with a list it never walks)
        assert not b256[0, 0][0] and b256[0, 0][1] == [True] * 4 + [False] * 4        # dead wavefronts inside a live 256-key block
        assert not b128[1, 1][0] and b128[1, 1][1] == [True, True, False, False]
        assert not any(b256[2, 0][1])
        t = AC.onepass_tables(st, True)
        assert t.qt_desc.tolist() == [[0, 64], [64, 64], [128, 64], [192, 56], [248, 8]] and t.kb_desc[:, :2].tolist() == [[0, 128], [128, 128]]
        state = AC.onepass_state(t, pad)
        assert state[0] == ([1], [0], [0, 1]) and state[4] == ([1], [0], [0, 1])      # unvisited query tiles, a dead key block
        assert state[1] == ([0, 1], [], []) and state[2] == ([0, 1], [], [])
        tp = AC.onepass_tables(st, False)
        assert len(tp.kb_desc) == 1 and len(tp.qt_desc) == 4
        for S in AC.SPLITS:                                                           # split mode: workgroups without a key block
            for tab in (t, tp):
                owners = [sid for sid in range(S) if any(kb % S == sid for kb in range(len(tab.kb_desc)))]
                assert len(owners) == min(S, len(tab.kb_desc))
                for sid in range(S):
                    for live_, dead_, unvisited in AC.onepass_state(tab, pad, S, sid):
                        assert sid in owners or (live_ == [] and dead_ == [] and unvisited == list(range(len(tab.qt_desc))))
        assert any(len(tab.kb_desc) < S for S in AC.SPLITS for tab in (t, tp))
    # ---- tail257
    st, pad = AC.structure("tail257"), AC.padding("tail257")
    N = st.n_tokens
    assert N == 257 and AC.nk_pad_of(N) == 512
    fl = AC.ktile_flags(pad)
    assert fl.shape == (3, 5) and fl[:, 4].tolist() == [1, 1, 1]                      # the one-key last tile is never "all valid"
    sc128, sc64_128, sc64_256 = st.attn_schedule(128, 64), st.attn_schedule(64, 128), st.attn_schedule(64, 256)
    assert (sc128.n_q, sc128.n_k) == (3, 5) and (sc64_128.n_q, sc64_128.n_k) == (5, 3) and sc64_256.n_k == 2
    live = AC.dq_live_lists(st, pad)
    assert live[1, 0] == [(0, True), (1, True), (2, False)]                           # unmasked and masked tiles of the SAME rows
    assert live[0, 0] == [(2, False)]                                                 # (key 128 is modality 0's last token)
    b128, b256 = AC.dkv_blocks(st, pad, 128), AC.dkv_blocks(st, pad, 256)
    assert b128[0, 0][0] and b128[1, 2][1] == [False, True, True, True] and b256[1, 1][1] == [False] + [True] * 7
    t, tp = AC.onepass_tables(st, True), AC.onepass_tables(st, False)
    assert t.qt_desc[:3].tolist() == [[0, 43], [43, 43], [86, 43]] and t.kb_desc[:, :2].tolist() == [[0, 129], [129, 128]]
    assert tp.qt_desc[-1].tolist() == [256, 1] and tp.kb_desc[-1, :2].tolist() == [256, 1] and len(tp.kb_desc) == 2
    # ---- tiny14
    st, pad = AC.structure("tiny14"), AC.padding("tiny14")
    assert st.n_tokens == 14 and AC.ktile_flags(pad).tolist() == [[1], [1], [1]]
    sc = st.attn_schedule(128, 64)
    assert (sc.n_q, sc.n_k) == (1, 1) and sc.q_full.tolist() == [0]
    assert len(AC.onepass_tables(st, True).kb_desc) == 1
    # ---- every case fits the one-pass kernels' tables (a refusal would be a failure), and every sample keeps its fusion tokens
    for case, variant in AC.SELF:
        st, pad = AC.structure(case, variant), AC.padding(case)
        assert not pad[:, -AC.CASES[case]["fusion"]:].any() and 3 <= pad.shape[0] <= 5
        for aligned in (True, False):
            t = AC.onepass_tables(st, aligned)
            assert len(t.qt_desc) < 256 and len(t.kb_desc) <= 64 and int(t.kb_desc[:, 3].max()) + 6 <= 256 and len(t.kb_qt) + 4 * len(t.kb_desc) <= 768
    for case, variant in AC.POOL:
        assert len(AC.structure(case, variant).qmask_pool) == 8


def test_padding_and_blocked_follow_the_listed_lengths():
    pad = AC.padding("aligned256")
    assert pad[0, :128].all() and not pad[0, 128:].any() and pad[1, 128:192].all() and pad[3].sum() == 256 - 8 - 3
    st = AC.structure("aligned256")
    blk = AC.blocked(st, pad)
    assert blk.shape == (5, 256, 256) and blk[0, :128].all() and not blk[2, 0, :128].any() and blk[2, 0, 128:].all()
    assert blk[0, 248:, :128].all() and not blk[2, 248, :248].all()


# ------------------------------------------------------------------------------------------- the emulation meets the bounds
def run_emulation(ops, dq_f32=False, **mut):
    q, k, v, d_o = U.head_operands(ops)
    o, lse = U.emulate_forward(q, k, v, ops["blk"])
    delta, dvmean = U.emulate_prep(d_o, o, lse, ops["N"])
    dq, dk, dv = U.emulate_backward(q, k, v, d_o, lse, delta, dvmean, ops["blk"], dq_f32=dq_f32, **mut)
    return dict(q=q, k=k, v=v, d_o=d_o, o=o, lse=lse, delta=delta, dvmean=dvmean, dq=dq, dk=dk, dv=dv)


def references(ops, e, dq_f32=False):
    fwd = U.forward_ref(e["q"], e["k"], e["v"], ops["blk"])
    bwd = U.backward_ref(e["q"], e["k"], e["v"], e["d_o"], e["lse"], e["delta"], e["dvmean"], ops["blk"], dq_f32=dq_f32)
    return fwd, bwd


@pytest.mark.parametrize("case,variant,pool", [(c, v, False) for c, v in AC.SELF] + [(c, v, True) for c, v in AC.POOL])
def test_emulation_meets_every_bound_with_room(case, variant, pool):
    ops = U.make_operands(case, variant, pool)
    worst = {}
    for dq_f32 in (False, True):
        e = run_emulation(ops, dq_f32)
        fwd, bwd = references(ops, e, dq_f32)
        assert float(fwd["lse_bound"].max()) < 1e-4, f"lse bound {float(fwd['lse_bound'].max())} log2 units"
        assert fwd["uniform"].any() or case == "tail257" and pool
        el, rw, el_l = U.check_forward(U.heads4(U.rows2(e["o"]), ops["b"]), e["lse"], fwd, "emulated forward")
        worst["o"] = (el, rw)
        d_ref, d_bound = U.delta_ref(e["d_o"], e["o"].double())
        U.check_elements(e["delta"], d_ref, d_bound, "emulated delta")
        v_ref, v_bound = U.dvmean_ref(e["d_o"], e["lse"], ops["N"])
        U.check_elements(e["dvmean"], v_ref, v_bound, "emulated dvmean", names=("sample", "head", "-", "column"))
        res = U.check_backward(e["dq"].double(), e["dk"].double(), e["dv"].double(), bwd, f"emulated backward (dq_f32={dq_f32})")
        for name, (el, rw) in res.items():
            worst[name + ("_f32" if dq_f32 and name == "dq" else "")] = (el, rw)
        assert el_l <= 1.0
    print(f"\n{case} {variant} pool={pool}: " + "  ".join(f"{n} {a:.2f}/{b_:.2f}" for n, (a, b_) in sorted(worst.items())))
    for name, (el, rw) in worst.items():
        assert el <= EMU_ELEMENT_MAX and rw <= EMU_ROW_MAX, f"{name}: emulation at {el:.3f} of the element bound, {rw:.3f} of the row bound"


def test_exact_zeros_where_the_bound_is_zero():
    """dk of a padded key and dq of a row without a visible key have a bound of exactly 0: only an exact 0 passes"""
    ops = U.make_operands("aligned256")
    e = run_emulation(ops)
    _, bwd = references(ops, e)
    assert float(bwd["dk_bound"][0, :, :128].max()) == 0 and float(bwd["dq_bound"][0, :, :128].max()) == 0
    assert float(bwd["dv_bound"][0, :, :128].min()) > 0          # (dvmean: sample 0 has uniform rows)
    dk = e["dk"].double().clone()
    dk[0, 1, 5, 9] = 1e-30
    with pytest.raises(AssertionError, match=r"dk: 1 of .*\(0, 1, 5, 9,"):
        U.check_backward(None, dk, e["dv"].double(), bwd, "mutant")


# ------------------------------------------------------------------------------------------- mutations
def test_one_row_with_lse_off_by_a_twentieth():
    ops = U.make_operands("aligned256")
    clean = run_emulation(ops)
    e = run_emulation(ops, lse_shift=(2, 1, 70, 0.05))
    _, bwd = references(ops, clean)          # (the reference is given the true lse, as a kernel's reference is given the forward's)
    with pytest.raises(AssertionError, match=r"dq: .*\(2, 1, 70, ") as exc:
        U.check_backward(e["dq"].double(), None, None, bwd, "mutant")
    assert len(set(re.findall(r"\((\d+, \d+, \d+), ", str(exc.value)))) == 1          # that row and no other
    # ... and the row check alone finds it when the element check is given twice its bound
    loose = dict(bwd, dq_bound=2.5 * bwd["dq_bound"])
    with pytest.raises(AssertionError, match=r"rows beyond .*\(2, 1, 70, "):
        U.check_rows(e["dq"].double(), loose["dq"], loose["dq_bound"], "mutant dq", row_limit=U.ROW_LIMIT / 2.5)
    U.check_backward(clean["dq"].double(), clean["dk"].double(), clean["dv"].double(), bwd, "clean")


def test_one_key_tile_left_out_of_one_row_block_of_dq():
    ops = U.make_operands("aligned256")
    clean = run_emulation(ops)
    e = run_emulation(ops, skip=(1, 0, 32, 32, 64, 64))          # sample 1, head 0, rows 32..63, keys 64..127
    _, bwd = references(ops, clean)
    with pytest.raises(AssertionError, match=r"dq: .*\(1, 0, (3[2-9]|[45]\d|6[0-3]), ") as exc:
        U.check_backward(e["dq"].double(), None, None, bwd, "mutant")
    rows = {int(r) for r in re.findall(r"\(1, 0, (\d+), \d+, ", str(exc.value))}
    assert rows and rows <= set(range(32, 64))


def test_dv_of_a_padded_key_without_dvmean():
    ops = U.make_operands("aligned256")
    e = run_emulation(ops)
    _, bwd = references(ops, e)
    assert bool(ops["pad"][0, 17]) and float(e["dvmean"][0, 1].abs().max()) > 0
    dv = e["dv"].double().clone()
    dv[0, 1, 17] -= e["dvmean"][0, 1, 0].double()
    with pytest.raises(AssertionError, match=r"dv: .*\(0, 1, 17, ") as exc:
        U.check_backward(None, e["dk"].double(), dv, bwd, "mutant")
    assert "first (sample, head, key, column" in str(exc.value)


def test_one_output_row_left_at_the_sentinel():
    ops = U.make_operands("tail257")
    e = run_emulation(ops)
    _, bwd = references(ops, e)
    b, N, D = ops["b"], ops["N"], ops["D"]
    out = G.guarded_out(b * N, D, D + 8, torch.bfloat16)
    val = U.rows2(e["dq"]).clone()
    keep = out.t[2 * N + 256].clone()
    out.t.copy_(val)
    out.t[2 * N + 256] = keep          # the one-row last tile of sample 2 is never stored
    with pytest.raises(AssertionError, match=r"dq: 128 of .*\(2, 0, 256, 0, nan"):
        U.check_backward(U.heads4(out.t, b), None, None, bwd, "mutant")
    G.assert_guard_intact(out)


@pytest.mark.parametrize("where", ["row N", "column D"])
def test_a_store_outside_a_guarded_output(where):
    ops = U.make_operands("tiny14")
    e = run_emulation(ops)
    _, bwd = references(ops, e)
    b, N, D = ops["b"], ops["N"], ops["D"]
    out = G.guarded_out(b * N, 3 * D, 3 * D + 8, torch.bfloat16)
    out.t[:, D:2 * D].copy_(U.rows2(e["dk"]))
    out.t[:, 2 * D:].copy_(U.rows2(e["dv"]))
    U.check_backward(None, U.heads4(out.t[:, D:2 * D], b), U.heads4(out.t[:, 2 * D:], b), bwd, "guarded")
    assert (out.t[:, :D].view(torch.int16) == -1).all()          # the q columns of the dk | dv matrix: still the sentinel
    G.assert_guard_intact(out)
    r, c = {"row N": (b * N, D), "column D": (3, 3 * D)}[where]
    wide = torch.as_strided(out.t, (b * N + 1, 3 * D + 8), (3 * D + 8, 1), out.t.storage_offset())
    wide[r, c] = 0.0
    with pytest.raises(AssertionError, match=rf"guard bytes overwritten.*\({r}, {c}\)"):
        G.assert_guard_intact(out)


def test_uniform_rows_and_nan_in_the_forward():
    ops = U.make_operands("aligned256", "zorro")
    e = run_emulation(ops)
    fwd, _ = references(ops, e)
    o4 = U.heads4(U.rows2(e["o"]), ops["b"])
    lse = e["lse"].clone()
    lse[0, 1, 3] = 0.0          # a uniform row not flagged
    with pytest.raises(AssertionError, match=r"uniform rows .*\[0, 1, 3\]"):
        U.check_forward(o4, lse, fwd, "mutant")
    lse = e["lse"].clone()
    lse[2, 0, 200] += 2e-4
    with pytest.raises(AssertionError, match=r"lse: 1 of .*\(2, 0, 200, "):
        U.check_forward(o4, lse, fwd, "mutant")
    o_bad = o4.clone()
    o_bad[4, 1, 255, 63] = float("nan")
    with pytest.raises(AssertionError, match=r"o: 1 of .*\(4, 1, 255, 63, nan"):
        U.check_forward(o_bad, e["lse"], fwd, "mutant")
