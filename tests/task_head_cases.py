"""Case table of the task-head kernel's edge tests (tests/test_task_head_cpu.py checks the table and the reference, tests/
test_task_head_gpu.py runs it).  Plain data, no torch.

The kernel (csrc/task_head.hip) gives one workgroup 64 rows and one wave a row, 16-byte accesses of 64 lanes x 4 trips over D:
b in {1, 5, 64, 65, 129} is one row, a partial wave round, exactly one workgroup, one row into the second and one row into the third;
D in {4, 128, 516, 1024} is one lane, half a trip, two trips and a lane's tail, and the limit; L in {1, 7, 64} one lane, a few, all."""
L1, MSE, BCE = 0, 1, 2
ROWS_PER_BLOCK = 64          # csrc/task_head.hip TH_ROWS

# presence: "null" = no presence words (any_bits 0), "all" = words given and every row valid, "mixed" = n_valid of the b rows valid,
# "none" = no valid row.  din: None, "given" (a second tensor) or "alias" (d_pooled is d_pooled_in).


def case(b, L, D, R, slot, loss, presence="null", n_valid=None, din=None, base=0.0, tw=1.0, acc=0, ld_extra=0, col_off=0):
    nv = {"null": b, "all": b, "none": 0}.get(presence, n_valid)
    assert 0 <= slot < R and 0 <= nv <= b and col_off <= ld_extra
    name = f"b{b}-L{L}-D{D}-R{R}s{slot}-{('l1', 'mse', 'bce')[loss]}-{presence}{nv if presence == 'mixed' else ''}" \
           f"-{din or 'nodin'}-acc{acc}" + (f"-ld+{ld_extra}@{col_off}" if ld_extra else "") + (f"-tw{tw}" if tw != 1.0 else "")
    return dict(name=name, b=b, L=L, D=D, R=R, slot=slot, loss=loss, presence=presence, n_valid=nv, din=din, base=base, tw=tw, acc=acc,
                ld_labels=L + ld_extra, col_off=col_off)


CASES = [
    # one row, one lane, one slot
    case(1, 1, 4, 1, 0, L1),
    case(1, 64, 1024, 5, 4, MSE, din="given", base=0.5),
    case(1, 7, 516, 5, 0, BCE, presence="all", acc=1),
    # a partial round of the four waves
    case(5, 7, 128, 5, 4, MSE, presence="mixed", n_valid=4, din="given", base=0.5, ld_extra=3, col_off=2),
    case(5, 1, 4, 5, 0, BCE, presence="mixed", n_valid=4, acc=1),
    case(5, 64, 516, 1, 0, L1, presence="mixed", n_valid=2, din="alias", base=0.5),
    # exactly one workgroup
    case(64, 64, 516, 5, 0, BCE, presence="all", din="alias", base=0.5),
    case(64, 1, 128, 5, 4, L1, presence="mixed", n_valid=32, acc=1, ld_extra=6, col_off=6),
    case(64, 7, 1024, 1, 0, MSE, tw=0.5),
    # one row into the second workgroup
    case(65, 1, 1024, 1, 0, MSE, presence="mixed", n_valid=64, acc=1),
    case(65, 7, 516, 5, 4, L1, presence="mixed", n_valid=33, din="alias", base=0.5),
    case(65, 64, 4, 5, 0, BCE, presence="mixed", n_valid=32, din="given", base=0.5, ld_extra=1, col_off=1),
    case(65, 64, 128, 1, 0, MSE, presence="null", din="given", base=0.5, tw=3.0),
    # three workgroups, the last with one row
    case(129, 7, 128, 5, 4, L1, presence="mixed", n_valid=128, din="given", base=0.5, acc=1),
    case(129, 64, 4, 5, 0, BCE, presence="mixed", n_valid=64, ld_extra=2, col_off=0),
    case(129, 1, 516, 1, 0, MSE, presence="mixed", n_valid=64),
    case(129, 64, 1024, 5, 4, MSE, presence="mixed", n_valid=128, din="alias", base=0.5, acc=1),
    case(129, 1, 128, 5, 0, BCE, presence="all", din="given", base=0.5, tw=0.5),
    # the one case without a valid row
    case(5, 7, 128, 5, 0, MSE, presence="none", din="given", base=0.5, ld_extra=3, col_off=1),
]

NO_VALID_ROW = [c["name"] for c in CASES if c["n_valid"] == 0]

# sizes the entry point and the workspace query refuse, by return code (no launch): (field, value, code name)
REFUSED_SIZES = [("b", 0, "BADARG"), ("R", 0, "BADARG"), ("D", 0, "BADARG"), ("L", 0, "BADARG"), ("slot", -1, "BADARG"), ("slot", 5, "BADARG"),
                 ("ld_labels", 6, "BADARG"), ("loss_type", 3, "BADARG"), ("loss_type", -1, "BADARG"), ("accumulate", 2, "BADARG"),
                 ("D", 1028, "UNSUPPORTED"), ("L", 65, "UNSUPPORTED"), ("D", 126, "ALIGN")]
REQUIRED_POINTERS = ["pooled", "w", "bias", "labels", "pred", "loss", "d_pooled", "gw", "gb", "workspace"]
WIDE_POINTERS = ["pooled", "w", "d_pooled", "d_pooled_in", "gw", "workspace"]          # 16-byte accesses
NARROW_POINTERS = ["bias", "labels", "pred", "loss", "gb", "present"]                  # 4-byte accesses
