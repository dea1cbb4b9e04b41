"""Case tables of the class-head kernels' edge tests (tests/test_class_head_cpu.py checks the tables and the reference, tests/
test_class_head_gpu.py runs them).  Plain data, no torch.

mca_class_head_fwd_bwd (csrc/class_head.hip) gives one workgroup 64 rows, one wave a row and one lane a class, 16-byte accesses of
64 lanes x 4 trips over D: b in {1, 5, 64, 65, 129} is one row, a partial wave round, exactly one workgroup, one row into the second
and one row into the third; D in {4, 128, 516, 1024} is one lane, half a trip, two trips and a lane's tail, and the limit; C in
{2, 7, 64} the smallest head, a few lanes, all lanes.  mca_probe_head_ce_f32 gives one workgroup four rows and walks K in trips of
64 lanes: B in {1, 4, 5}, K in {1, 64, 65, 1024}, C in {2, 3, 64}."""
ROWS_PER_BLOCK = 64          # csrc/class_head.hip CH_ROWS

# presence: "null" = no presence words (any_bits 0), "all" = words given and every row valid, "mixed" = n_valid of the b rows valid,
# "none" = no valid row.  unlabelled: how many of the VALID rows carry the label -1 ("all": every one).  cw: None (NULL) or "zero1"
# (weights given, the weight of class 1 is 0).  din: None, "given" (a second tensor) or "alias" (d_pooled is d_pooled_in).
# w_scale: the head's weights times this power of two (logits of magnitude ~200 at 16).  junk: the labels of rows that are invalid by
# presence hold NaN and values >= C in turn (else NaN alone).


def case(b, C, D, R, slot, presence="null", n_valid=None, unlabelled=0, cw=None, eps=0.0, din=None, base=0.0, tw=1.0, acc=0, ld=1, col_off=0,
         w_scale=1, junk=False):
    nv = {"null": b, "all": b, "none": 0}.get(presence, n_valid)
    nu = nv if unlabelled == "all" else unlabelled
    assert 0 <= slot < R and 0 <= nv <= b and 0 <= nu <= nv and col_off < ld
    name = f"b{b}-C{C}-D{D}-R{R}s{slot}-{presence}{nv if presence == 'mixed' else ''}-u{nu}-{cw or 'nocw'}-eps{eps}-{din or 'nodin'}-acc{acc}" \
           + (f"-ld{ld}@{col_off}" if ld > 1 else "") + (f"-tw{tw}" if tw != 1.0 else "") + (f"-wx{w_scale}" if w_scale != 1 else "") \
           + ("-junk" if junk else "")
    return dict(name=name, b=b, C=C, D=D, R=R, slot=slot, presence=presence, n_valid=nv, n_unlabelled=nu, cw=cw, eps=eps, din=din, base=base,
                tw=tw, acc=acc, ld_labels=ld, col_off=col_off, w_scale=w_scale, junk=junk)


CASES = [
    # one row
    case(1, 2, 4, 1, 0),
    case(1, 64, 1024, 5, 4, din="given", base=0.5, eps=0.1),
    case(1, 7, 516, 5, 0, presence="all", acc=1, cw="zero1"),
    # a partial round of the four waves
    case(5, 7, 128, 5, 4, presence="mixed", n_valid=4, unlabelled=1, din="given", base=0.5, ld=4, col_off=2),
    case(5, 2, 4, 5, 0, presence="mixed", n_valid=4, acc=1, eps=0.1, cw="zero1"),
    case(5, 64, 516, 1, 0, presence="mixed", n_valid=3, din="alias", base=0.5, tw=0.5),
    # exactly one workgroup
    case(64, 64, 516, 5, 0, presence="all", unlabelled=21, din="alias", base=0.5, cw="zero1", eps=0.1),
    case(64, 2, 128, 5, 4, presence="mixed", n_valid=32, unlabelled=5, acc=1, ld=7, col_off=6),
    case(64, 7, 1024, 1, 0, tw=0.5, eps=0.1),
    # one row into the second workgroup
    case(65, 2, 1024, 1, 0, presence="mixed", n_valid=64, acc=1, cw="zero1"),
    case(65, 7, 516, 5, 4, presence="mixed", n_valid=33, unlabelled=11, din="alias", base=0.5, eps=0.1),
    case(65, 64, 4, 5, 0, presence="mixed", n_valid=32, din="given", base=0.5, ld=2, col_off=1, cw="zero1"),
    case(65, 64, 128, 1, 0, presence="null", unlabelled=20, din="given", base=0.5, tw=3.0),
    # three workgroups, the last with one row
    case(129, 7, 128, 5, 4, presence="mixed", n_valid=128, unlabelled=40, din="given", base=0.5, acc=1, cw="zero1", eps=0.1, tw=0.5),
    case(129, 64, 4, 5, 0, presence="mixed", n_valid=64, ld=3, col_off=0, eps=0.1),
    case(129, 2, 516, 1, 0, presence="mixed", n_valid=64, unlabelled=3),
    case(129, 64, 1024, 5, 4, presence="mixed", n_valid=128, din="alias", base=0.5, acc=1, cw="zero1"),
    case(129, 7, 128, 5, 0, presence="all", din="given", base=0.5, tw=0.5),
    # nothing counted: no valid row; every valid row unlabelled (with and without accumulate)
    case(5, 7, 128, 5, 0, presence="none", din="given", base=0.5, ld=4, col_off=1),
    case(65, 7, 128, 5, 4, presence="mixed", n_valid=40, unlabelled="all", din="given", base=0.5, cw="zero1", eps=0.1),
    case(5, 2, 4, 1, 0, unlabelled="all", acc=1),
    # logits of magnitude ~200: expf overflows unless the row maximum is subtracted first
    case(65, 7, 128, 5, 4, presence="mixed", n_valid=60, unlabelled=7, din="given", base=0.5, w_scale=16, eps=0.1, cw="zero1"),
    # rows that are invalid by presence carry NaN labels and labels >= C
    case(65, 7, 128, 5, 0, presence="mixed", n_valid=33, unlabelled=4, ld=3, col_off=1, junk=True),
]

NOTHING_COUNTED = [c["name"] for c in CASES if c["n_valid"] == c["n_unlabelled"]]
LARGE_LOGITS = [c["name"] for c in CASES if c["w_scale"] != 1]

# sizes mca_class_head_fwd_bwd refuses, by return code (no launch): (field, value, code name)
REFUSED_SIZES = [("b", 0, "BADARG"), ("R", 0, "BADARG"), ("D", 0, "BADARG"), ("C", 1, "BADARG"), ("C", 0, "BADARG"), ("slot", -1, "BADARG"),
                 ("slot", 5, "BADARG"), ("ld_labels", 0, "BADARG"), ("label_smoothing", 1.0, "BADARG"), ("label_smoothing", -0.1, "BADARG"),
                 ("label_smoothing", float("nan"), "BADARG"), ("accumulate", 2, "BADARG"), ("D", 1028, "UNSUPPORTED"), ("C", 65, "UNSUPPORTED"),
                 ("D", 126, "ALIGN")]
REQUIRED_POINTERS = ["pooled", "w", "bias", "labels", "pred", "loss", "d_pooled", "gw", "gb", "workspace"]
WIDE_POINTERS = ["pooled", "w", "d_pooled", "d_pooled_in", "gw", "workspace"]                  # 16-byte accesses
NARROW_POINTERS = ["bias", "labels", "class_weights", "pred", "loss", "gb", "present"]         # 4-byte accesses


# ---- mca_probe_head_ce_f32 ---------------------------------------------------------------------------------------------------
def probe_case(B, C, K, aidx=False, yidx=False, dz=True, da=False, ldy=1, bad=False):
    """bad: batch row 1 carries the label C and batch row 2 the label 0.5 (no class indices: loss 0 and dz 0 there, the divisor stays B)"""
    assert not bad or B >= 4
    name = f"B{B}-C{C}-K{K}" + ("-aidx" if aidx else "") + ("-yidx" if yidx else "") + ("" if dz else "-eval") + ("-da" if da else "") \
           + (f"-ldy{ldy}" if ldy > 1 else "") + ("-bad" if bad else "")
    return dict(name=name, B=B, C=C, K=K, aidx=aidx, yidx=yidx, dz=dz, da=da, ldy=ldy, bad=bad)


PROBE_CASES = [
    probe_case(1, 2, 1),
    probe_case(1, 64, 1024, aidx=True, yidx=True, da=True),
    probe_case(1, 3, 65, dz=False),
    probe_case(4, 3, 64, aidx=True, yidx=True, ldy=3),
    probe_case(4, 64, 65, da=True),
    probe_case(4, 2, 1024, dz=False, yidx=True, ldy=2),
    probe_case(5, 3, 1, aidx=True, yidx=True),
    probe_case(5, 2, 64, da=True, ldy=5, bad=True),
    probe_case(5, 64, 1024, aidx=True, yidx=True, da=True),
    probe_case(5, 3, 65, dz=False, aidx=True),
]
# (argument, value, code name): sizes mca_probe_head_ce_f32 refuses without a launch
PROBE_REFUSED = [("B", 0, "BADARG"), ("K", 0, "BADARG"), ("C", 1, "BADARG"), ("lda", "K-1", "BADARG"), ("ldy", 0, "BADARG"),
                 ("K", 1025, "UNSUPPORTED"), ("C", 65, "UNSUPPORTED")]
PROBE_REQUIRED_POINTERS = ["a", "w", "bias", "labels", "pred", "loss_part"]
