"""The cases of the attention edge tests, in one place and importable without a GPU: tests/test_attention_edges_gpu.py runs
them through the C ABI, tests/test_attention_edges_cpu.py asserts from the schedules (structure.build_schedule /
build_onepass_schedule) and a numpy restatement of the ktile_flags rule that each case reaches what it is listed for.

Every case: 2 heads, fusion_combos_powers (3, 2), the valid length of every modality in every sample LISTED (one sample per
row of `lengths`), fusion tokens never padded.  Tile and padding edges the workload shapes never put on a multiple of 64 / 128:

  aligned256  [128, 64, 56] + 8 fusion tokens, N = 256 = nk_pad, MCA (fcl) and Zorro
      sample 0 (0, 64, 56)   : the 128-row query tile 0 of the dq pass has an EMPTY live list, the 128-key block 0 of the dkv pass
                               is dead, the first four wavefronts of its 256-key block are dead, the structure-aligned one-pass
                               table has two query tiles nobody visits and a dead key block
      sample 1 (128, 0, 56)  : key tile 2 is dead inside live key blocks
      sample 2 (128, 64, 56) : every key tile is all-valid: the unmasked fast path (a structurally full tile of flag 2) next to
                               masked tiles
      sample 3 (1, 1, 1), sample 4 (0, 0, 0): one key per modality / only the fusion tokens
  tail257     [129, 64, 56] + 8, N = 257, MCA: a one-key last key tile, 128-key block and 256-key block, a one-row 128-row query
              tile and 64-row dkv step, nk_pad = 512; the plain one-pass grid has a 1-row tile and a 1-key block, the aligned one
              43-row tiles and a 129-key block
  tiny14      [5, 3, 2] + 4, N = 14, MCA: everything inside one partial tile"""
import importlib

import numpy as np

HEADS = 2
DH = 64
POWERS = (3, 2)

CASES = {
    "aligned256": dict(dims=[128, 64, 56], fusion=8, variants=("mca", "zorro"), pool=True, seed=101,
                       lengths=[(0, 64, 56), (128, 0, 56), (128, 64, 56), (1, 1, 1), (0, 0, 0)]),
    "tail257": dict(dims=[129, 64, 56], fusion=8, variants=("mca",), pool=True, seed=102,
                    lengths=[(0, 64, 56), (129, 64, 56), (129, 1, 0)]),
    "tiny14": dict(dims=[5, 3, 2], fusion=4, variants=("mca",), pool=False, seed=103,
                   lengths=[(5, 3, 2), (0, 3, 1), (0, 0, 0)]),
}
# (case, variant) of the self-attention tests; (case, variant) of the pooling tests (nq = 8 return tokens, q_bstride = 0)
SELF = [(c, v) for c, d in CASES.items() for v in d["variants"]]
POOL = [(c, "mca") for c, d in CASES.items() if d["pool"]]
SPLITS = (2, 4, 8)          # mca_attn_bwd_onepass split mode; cases with 2 key blocks: 4 and 8 leave workgroups without a key block


def structure(case, variant="mca"):
    S = importlib.import_module("mca-paper_amd.structure")
    c = CASES[case]
    return S.FusionStructure(list(c["dims"]), c["fusion"], POWERS, fcl=variant == "mca", zorro=variant == "zorro")


def padding(case):
    """(b, N) bool, True = padded key: the valid prefix of every modality as listed, fusion tokens valid"""
    c = CASES[case]
    n = sum(c["dims"]) + c["fusion"]
    pad = np.zeros((len(c["lengths"]), n), bool)
    for s, lens in enumerate(c["lengths"]):
        off = 0
        for dim, ln in zip(c["dims"], lens):
            assert 0 <= ln <= dim
            pad[s, off + ln:off + dim] = True
            off += dim
    return pad


def nk_pad_of(n):
    return (n + 255) // 256 * 256


def ktile_flags(pad):
    """mca_build_keyinfo's rule per (sample, 64-key tile): 0 no valid key, 2 all 64 keys exist and are valid, else 1"""
    b, n = pad.shape
    nt = (n + 63) // 64
    fl = np.zeros((b, nt), np.uint8)
    for t in range(nt):
        valid = (~pad[:, t * 64:(t + 1) * 64]).sum(1)
        in_tile = min(64, n - t * 64)
        fl[:, t] = np.where(valid == 0, 0, np.where((valid == 64) & (in_tile == 64), 2, 1))
    return fl


def blocked(st, pad, pool=False):
    """(b, nq, N) bool: the pair is structurally blocked or the key is padded"""
    dense = st.dense_pool_mask() if pool else st.dense_attn_mask()
    return dense[None] | pad[:, None, :]


# ---- what the kernels do with a case, restated from their code (attention_bwd2.hip, attention_bwd1.hip)
def dq_live_lists(st, pad, pool=False):
    """per (sample, 128-row query tile) the dq pass's live list [(key tile, unmasked)]: the schedule's entries whose tile flag is
    not 0; unmasked = structurally full and flag 2"""
    sc = st.pool_schedule(128, 64) if pool else st.attn_schedule(128, 64)
    fl = ktile_flags(pad)
    out = {}
    for s in range(pad.shape[0]):
        for qt in range(sc.n_q):
            ent = range(sc.q_ptr[qt], sc.q_ptr[qt + 1])
            out[s, qt] = [(int(sc.q_kt[i]), bool(sc.q_full[i]) and fl[s, sc.q_kt[i]] == 2) for i in ent if fl[s, sc.q_kt[i]] != 0]
    return out


def dkv_blocks(st, pad, bkeys, pool=False):
    """per (sample, key block of bkeys keys) of the dkv pass: (dead block: every 64-key tile of it has flag 0, [wavefront dead] for
    its bkeys / 32 wavefronts of 32 keys, query steps listed)"""
    sc = st.pool_schedule(64, bkeys) if pool else st.attn_schedule(64, bkeys)
    fl = ktile_flags(pad)
    b, n = pad.shape
    out = {}
    for s in range(b):
        for kb in range(sc.n_k):
            tiles = [t for t in range(kb * bkeys // 64, (kb + 1) * bkeys // 64) if t < fl.shape[1]]
            dead = all(fl[s, t] == 0 for t in tiles)
            waves = []
            for w in range(bkeys // 32):
                keys = np.arange(kb * bkeys + w * 32, kb * bkeys + w * 32 + 32)
                waves.append(bool(all(k >= n or pad[s, k] for k in keys)))
            out[s, kb] = (dead, waves, int(sc.k_ptr[kb + 1] - sc.k_ptr[kb]))
    return out


def onepass_tables(st, aligned):
    S = importlib.import_module("mca-paper_amd.structure")
    return S.build_onepass_schedule(st.qmask_attn, st.kgroup, 64, 256, aligned)


def onepass_state(sc, pad, split=1, sid=0):
    """per sample of one workgroup (slice sid of `split`) of the one-pass kernels: (key blocks it sweeps, key blocks it writes as
    dead: dK = 0, dV = dvmean, query tiles it never visits: dq, or its slice of the partials, = 0)"""
    fl = ktile_flags(pad)
    out = []
    for s in range(pad.shape[0]):
        live, dead = [], []
        for kb, (k0, kn, _, _) in enumerate(sc.kb_desc.tolist()):
            if kb % split != sid:
                continue
            (live if any(fl[s, t] for t in range(k0 >> 6, ((k0 + kn - 1) >> 6) + 1)) else dead).append(kb)
        unvisited = [qt for qt in range(len(sc.qt_desc)) if not any(sc.visit[kb, qt] for kb in live)]
        out.append((live, dead, unvisited))
    return out
