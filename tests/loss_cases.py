"""The listed cases of the contrastive-loss edge tests (tests/test_loss_edges_gpu.py; tests/test_loss_edges_cpu.py shows without a
GPU that every case reaches the path it is listed for and that every bound is satisfiable).  Nothing here is drawn: the lists are
crosses of the sizes at which the five kernels of csrc/loss.hip change path, written out by the loops below.

A case: B gathered rows of R slots of D columns, b_local rows per rank (W = B / b_local ranks, every one of them is launched), a
list of terms (slot_a, slot_b, and_bits, or_bits) or the name of a small-config schedule ("schedule:mca"), the present word of
every row (the formula below, then the case's overrides) and the kind of data:
    exact    pooled integers in {-3 .. 3}, logit_scale 0: every logit is an exact fp32 integer; rows 0 and B - 1 are all 3, so row 0
             and column 0 of every Gram matrix have their maximum twice
    prod3    pooled ~ randn scaled so that max |T G| = 1e3 at logit_scale = ln(1 / 0.07): production magnitude at initialisation
    prod4    max |T G| = 1e4 at logit_scale = ln 100, the upper end of the clamp
"""
LT, ROWSTATS_BLOCK, DGRAM_BLOCK, DGRAM_MAX_GRID, DPOOLED_COLS, DPOOLED_SLICES, REDUCE_BLOCK = 16, 256, 256, 1024, 128, 4, 256
LDS_LIMIT = 60000          # bytes of dynamic LDS mca_contrastive_fwd_bwd allows reduce_terms_kernel: 3 T W floats


def cdiv(a, b):
    return (a + b - 1) // b


def present_word(i):
    """1 .. 7: every non-empty set of three modalities, in an order that is no multiple of a tile"""
    return 1 + (i * 5 + 3) % 7


# (slot_a, slot_b, and_bits, or_bits) over R = 3 slots: an and-only term, an or-only term, a term every row is valid for
TERMS3 = [(0, 2, 0b001, 0), (1, 2, 0, 0b110), (0, 1, 0, 0)]
# over R = 4 slots: slot 1 is slot_b of term 0 and slot_a of term 1, term 2 has slot_a == slot_b, slot 3 is named by no term
TERMS_DPOOLED = [(0, 1, 0b001, 0), (1, 2, 0, 0b011), (2, 2, 0, 0)]


def terms60():
    """the 60 terms of the largest schedule's size over 6 slots: and-only, or-only and combined conditions, none unconditional"""
    bits = [(1, 0), (2, 0), (4, 0), (3, 0), (0, 6), (0, 5), (1, 6), (4, 3), (0, 4), (5, 0)]
    return [(t % 6, (t // 6 + 2 * t + 1) % 6, *bits[t % 10]) for t in range(60)]


def _case(family, B, D, R, b_local, terms, kind, present=None, **kw):
    T = len(terms) if isinstance(terms, list) else None
    slots = "" if R is None else f"R{R}"          # a schedule brings its own slot count
    name = f"{family}-B{B}D{D}{slots}b{b_local}-{kind}" + (f"-{kw.pop('tag')}" if "tag" in kw else "")
    c = dict(name=name, family=family, B=B, D=D, R=R, b_local=b_local, terms=terms, T=T, kind=kind, present=present or {})
    c.update(kw)
    return c


CASES = []
PROD = ["prod3", "prod4"]
# ---- Gram tiles and D staging: one tile short, one full, one full + a tail of 1, two full + a tail of 1; the same for the 16-wide
# staging of D.  Every shape with exact logits, and with the two production magnitudes in turn.
n = 0
for B in (1, 15, 16, 17, 33):
    for D in (1, 15, 16, 17, 130):
        for b_local in [B] + ([B // 3] if B % 3 == 0 else []):
            CASES.append(_case("gram", B, D, 3, b_local, TERMS3, "exact"))
            CASES.append(_case("gram", B, D, 3, b_local, TERMS3, PROD[n % 2]))
            n += 1
# ---- rowstats: the 256-strided loops make one trip, exactly one, and a second one of one element
for B in (255, 256, 257):
    for kind in ("exact", "prod3", "prod4"):
        CASES.append(_case("rowstats", B, 8, 3, B, TERMS3[:2], kind))
CASES.append(_case("rowstats", 255, 8, 3, 85, TERMS3[:2], "exact"))
# ---- dgram: 513^2 = 263169 > 1024 x 256 = 262144 elements: the grid-stride loop makes a second pass of 1025 elements
CASES.append(_case("dgram", 513, 4, 2, 513, [(0, 1, 0b001, 0)], "exact"))
CASES.append(_case("dgram", 513, 4, 2, 513, [(0, 1, 0, 0b110)], "prod3"))
CASES.append(_case("dgram", 513, 4, 2, 171, [(0, 1, 0b010, 0)], "exact"))
# ---- dpooled: the 128-column loop around one and two trips and into a third; B = 1 .. 5: the four slices hold 0 or 1 or 2 addends
n = 0
for D in (127, 128, 129, 257):
    for B in (1, 2, 3, 4, 5):
        for b_local in [B] + ([B // 2] if B == 4 else []):
            CASES.append(_case("dpooled", B, D, 4, b_local, TERMS_DPOOLED, "exact"))
            CASES.append(_case("dpooled", B, D, 4, b_local, TERMS_DPOOLED, PROD[n % 2]))
            n += 1
# ---- reduce_terms: T W = 300 > 256.  Rank 1 (rows 2, 3) lacks modality 2: the terms that need it have no valid row there.  Rank 3
# (rows 6, 7) has present words of 0: no term has a valid row.  Rank 2 has every term.  Row 9: a word of 0 next to a live row.
P60 = {2: 0b011, 3: 0b001, 4: 0b111, 5: 0b111, 6: 0, 7: 0, 9: 0}
for kind in ("exact", "prod3"):
    CASES.append(_case("reduce", 10, 5, 6, 2, terms60(), kind, present=P60))
# row0 at every rank for W = 1, 2, 3; rank 0 of W = 3 sees only modality 1: the and-only term is NaN there and on no other rank
for b_local in (6, 3, 2):
    for kind in ("exact", "prod4"):
        CASES.append(_case("ranks", 6, 7, 3, b_local, TERMS3, kind, present={0: 0b010, 1: 0b010}))
# ---- the LDS limit: T W = 5000 floats x 3 = 60000 bytes, the largest the entry point accepts
CASES.append(_case("ldslimit", 100, 3, 3, 1, [TERMS3[t % 3] for t in range(50)], "exact"))
CASES.append(_case("ldslimit", 100, 3, 3, 1, [TERMS3[t % 3] for t in range(50)], "prod3"))
LDS_REFUSED = dict(T=56, B=90, b_local=1)          # T W = 5040: 60480 bytes
# ---- the schedules of structure.loss_terms for the three small configurations (tests/util_small.py) at B = 17
for variant in ("mca", "bimodal", "zorro"):
    for kind in ("exact", "prod3"):
        CASES.append(_case("schedule", 17, 16, None, 17, f"schedule:{variant}", kind, tag=variant))

assert len({c["name"] for c in CASES}) == len(CASES)


def paths(c, T):
    """what the launch code of mca_contrastive_fwd_bwd and the kernels' loops do with a case: restated from csrc/loss.hip"""
    B, D, W = c["B"], c["D"], c["B"] // c["b_local"]
    gx = min(cdiv(B * B, DGRAM_BLOCK), DGRAM_MAX_GRID)
    return dict(gram_tiles=cdiv(B, LT), gram_tail=B % LT, d_trips=cdiv(D, LT), d_tail=D % LT,
                rowstats_trips=cdiv(B, ROWSTATS_BLOCK),
                dgram_grid=gx, dgram_passes=cdiv(B * B, gx * DGRAM_BLOCK),
                dpooled_trips=cdiv(D, DPOOLED_COLS), dpooled_slices=[len(range(s, B, DPOOLED_SLICES)) for s in range(DPOOLED_SLICES)],
                reduce_trips=cdiv(T * W, REDUCE_BLOCK), lds_bytes=3 * T * W * 4, W=W)
