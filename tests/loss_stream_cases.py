"""The listed cases of the streaming contrastive-loss tests (tests/test_loss_stream_gpu.py; tests/test_loss_stream_cpu.py shows
without a GPU that every case reaches the path it is listed for and that every derived bound is satisfiable).  Nothing is drawn: the
lists are crosses of the sizes at which the kernels of csrc/loss_stream.hip change path.  A case is what tests/loss_cases.py
describes (B, D, R, b_local, terms, present overrides, kind of data); its helpers make the data.

TI owner rows of a block, TJ other-side rows of a tile step (4 waves x 32), TK columns of D staged per step, DMAX the largest D
accepted; tests/test_loss_stream_cpu.py holds them against mca_dbg_contrastive_stream_layout."""
import loss_cases as LC
from loss_cases import TERMS3, TERMS_DPOOLED, P60, terms60, cdiv, _case

TI, TJ, TK, DMAX = 32, 128, 32, 512
LANES = 8          # partial statistics of an owner row: 4 waves x 2 lane halves

CASES = []
PROD = ["prod3", "prod4"]
BS = [1, TI - 1, TI, TI + 1, 2 * TI + 1, TJ - 1, TJ, TJ + 1, 2 * TJ + 1]
DS = [d for d in (1, TK - 1, TK, TK + 1, 130) if 1 <= d <= DMAX]
# ---- strips, tiles and D staging: B around the strip and the tile, D around the staged chunk; every shape with exact logits and
# with the two production magnitudes in turn; b_local = B and B / 3 (ranks whose row0 is no multiple of a strip)
n = 0
for B in BS:
    for D in DS:
        for b_local in [B] + ([B // 3] if B % 3 == 0 else []):
            CASES.append(_case("tiles", B, D, 3, b_local, TERMS3, "exact"))
            CASES.append(_case("tiles", B, D, 3, b_local, TERMS3, PROD[n % 2]))
            n += 1
# ---- the widths the model uses, once each: D = 128 fills one wave's columns, D = 512 all sixteen sub-tiles
CASES.append(_case("width", 33, 128, 4, 33, TERMS_DPOOLED, "prod3"))
CASES.append(_case("width", 33, 512, 4, 11, TERMS_DPOOLED, "exact"))
CASES.append(_case("width", 33, 512, 4, 33, TERMS_DPOOLED, "prod4"))
# ---- a slot that several terms name, as slot_a and as slot_b, slot_a == slot_b, and a slot that no term names
n = 0
for B in (5, TI + 1, TJ + 1):
    for D in (TK + 1, 130):
        for b_local in [B] + ([B // 3] if B % 3 == 0 else []):
            CASES.append(_case("slots", B, D, 4, b_local, TERMS_DPOOLED, "exact"))
            CASES.append(_case("slots", B, D, 4, b_local, TERMS_DPOOLED, PROD[n % 2]))
            n += 1
# ---- 60 terms, ranks with dead terms and a rank with none (tests/loss_cases.py, "reduce")
for kind in ("exact", "prod3"):
    CASES.append(_case("reduce", 10, 5, 6, 2, terms60(), kind, present=P60))
    CASES.append(_case("reduce", 10, 5, 6, 10, terms60(), kind, present=P60))
for b_local in (6, 3, 2):
    for kind in ("exact", "prod4"):
        CASES.append(_case("ranks", 6, 7, 3, b_local, TERMS3, kind, present={0: 0b010, 1: 0b010}))
# ---- one row per rank at more ranks than the dense kernel's LDS holds (T W = 5040)
CASES.append(_case("manyranks", 90, 3, 3, 1, [TERMS3[t % 3] for t in range(56)], "exact"))
# ---- the schedules of structure.loss_terms for the three small configurations
for variant in ("mca", "bimodal", "zorro"):
    for kind in ("exact", "prod3"):
        CASES.append(_case("schedule", TI + 1, TK + 1, None, TI + 1, f"schedule:{variant}", kind, tag=variant))

assert len({c["name"] for c in CASES}) == len(CASES)

# the production shape: the CMU schedule (4 modalities, 11 combinations: 14 terms over 15 slots) at B = 1024, D = 512
PRODUCTION = dict(B=1024, D=512, b_local=1024, kind="prod3")


def cmu_terms():
    """(terms, R) of the CMU model's schedule (configs/CMU_config1.yaml: four modalities, fcl)"""
    import importlib
    S = importlib.import_module("mca-paper_amd.structure")
    st = S.FusionStructure([1500, 450, 450, 50], 88, (4, 3, 2), fcl=True, zorro=False)
    terms = S.loss_terms(["a", "b", "c", "d"], st, False, False)
    return [(t.slot_a, t.slot_b, t.and_bits, t.or_bits) for t in terms], st.n_return


def paths(c, T):
    """what the launch code of mca_contrastive_stream_fwd_bwd and the kernels' loops do with a case: restated from csrc/loss_stream.hip"""
    B, D, b = c["B"], c["D"], c["b_local"]
    return dict(strips=cdiv(B, TI), strip_tail=B % TI, tiles=cdiv(B, TJ), tile_tail=B % TJ, k_trips=cdiv(D, TK), k_tail=D % TK,
                grad_strips=cdiv(b, TI), grad_tail=b % TI, row0_aligned=b % TI == 0, waves_with_columns=cdiv(D, DMAX // 4),
                subtiles=cdiv(D, 32), W=B // b, accepted=1 <= D <= DMAX, dense_lds_bytes=3 * T * (B // b) * 4)
