"""The listed cases of the row-kernel edge tests (tests/test_row_edges_gpu.py), each LayerNorm case with the plan it must reach:
tests/test_row_edges_cpu.py asks the library's planners (csrc/ln_plan.h through mca_dbg_plan_layernorm_fwd / _bwd) without a GPU.
Nothing here is drawn: the lists are crosses of the sizes at which the kernels change path, written out by the loops below.

A case's plan is stated by the family that lists it (form and width) and by the grid rules restated below (docs/parity.md lists
them); the literal plans at the end pin those rules to numbers written down.  Offsets (x_off, gamma_off, ybf_off, dxb_off) are bytes past a
16-byte boundary."""
NONE, NARROW, TRUNK, GENERAL, PARAMS = range(5)          # hip.LN_*
PACK_EXTRA = 5                                           # rows between two samples of a packed placement: y_bstride = (period + 5) ld


def cdiv(a, b):
    return (a + b - 1) // b


def up(a, b):
    return cdiv(a, b) * b


COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]


# ================================================================================================ LayerNorm forward
def _fwd(name, rows, cols, form, width, **kw):
    c = dict(name=name, rows=rows, cols=cols, ldx=cols + 3, x_off=0, gamma_off=0, add_off=0, beta=0, mask=0, add=0, period=0, y=0, ldy=cols + 1,
             y_row0=0, ybf=1, ld_bf16=0, ybf_off=0, cols_pad=cols, stats=1, knobs={})
    c.update(kw)
    if c["ybf"] and not c["ld_bf16"]:
        c["ld_bf16"] = max(cols, c["cols_pad"]) + 5
    if form == NARROW:
        grid = min(cdiv(rows, 16), 4096)
        passes = cdiv(rows, grid * 16)
    elif form == TRUNK:
        grid, passes = cdiv(rows, 8), 1
    else:
        grid = min(cdiv(rows, 4), 8192)
        passes = cdiv(rows, grid * 4)
    c["plan"] = dict(form=form, width=width, grid_x=grid, passes=passes)
    return c


def _wide_pad(cols):
    return up(cols, 8) + 8


LN_FWD = []
# ---- narrow: 16 lanes per row.  cols around the 16-lane stride and at its 256 limit, rows around the 16 rows of a workgroup
for ci, cols in enumerate([1, 15, 16, 17, 74, 255, 256]):
    for ri, rows in enumerate([1, 15, 17, 33]):
        for v in range(2):
            beta, mask = COMBOS[(ci + ri + v) % 4]
            pad = cols if v == (ci + ri) % 2 else _wide_pad(cols)
            LN_FWD.append(_fwd(f"narrow-{cols}x{rows}-b{beta}m{mask}-pad{pad}", rows, cols, NARROW, 0, beta=beta, mask=mask, cols_pad=pad))
LN_FWD.append(_fwd("narrow-second-pass", 16 * 4096 + 17, 1, NARROW, 0, beta=1, mask=1, cols_pad=16))
# ---- the narrow / general boundary
LN_FWD += [
    _fwd("edge-256-narrow", 9, 256, NARROW, 0, beta=1, ldx=260, ld_bf16=264),
    _fwd("edge-257-general-scalar", 9, 257, GENERAL, 1, beta=1),
    _fwd("edge-260-general-vector", 9, 260, GENERAL, 4, beta=1, ldx=264, ld_bf16=264),
    _fwd("edge-256-knob12-general", 9, 256, GENERAL, 4, beta=1, ldx=260, ld_bf16=264, knobs={12: 1}),
]
# ---- trunk: two rows per wavefront, eight per workgroup; and what an operand 4 bytes off a 16-byte boundary does to it
# (a 256-column call that fits the trunk form fits the narrow form too, and the narrow rule is asked first: ln_fwd_trunk_kernel<1> is
# never launched by the forward, and neither misalignment moves such a call off the narrow kernel, which reads and stores scalars)
for cols in (256, 512, 1024):
    trunk, gvec, gsc = ((NARROW, 0),) * 3 if cols == 256 else ((TRUNK, cols // 256), (GENERAL, 4), (GENERAL, 1))
    for rows in (1, 2, 7, 8, 9):
        for stats in (1, 0):
            LN_FWD.append(_fwd(f"trunk-{cols}x{rows}-stats{stats}", rows, cols, *trunk, ldx=cols + 4, ld_bf16=cols + 8, stats=stats))
        LN_FWD.append(_fwd(f"trunk-{cols}x{rows}-gamma+4", rows, cols, *gvec, ldx=cols + 4, ld_bf16=cols + 8, gamma_off=4))
        LN_FWD.append(_fwd(f"trunk-{cols}x{rows}-x+4", rows, cols, *gsc, ldx=cols + 4, ld_bf16=cols + 8, x_off=4))
# ---- general, vector: y only, y_bf16 only (beta and an add table keep it off the narrow and trunk forms), both
for ci, cols in enumerate([4, 252, 260, 1020, 1024]):
    for ri, rows in enumerate([1, 3, 4, 5]):
        mask = (ci + ri) % 2
        LN_FWD.append(_fwd(f"vec-{cols}x{rows}-y", rows, cols, GENERAL, 4, ldx=cols + 4, y=1, ldy=cols + 8, ybf=0, mask=mask, beta=1 - mask, add=mask))
        LN_FWD.append(_fwd(f"vec-{cols}x{rows}-ybf", rows, cols, GENERAL, 4, ldx=cols + 4, ld_bf16=cols + 12, cols_pad=cols + 8, mask=mask, beta=1, add=1))
        LN_FWD.append(_fwd(f"vec-{cols}x{rows}-both", rows, cols, GENERAL, 4, ldx=cols + 8, y=1, ldy=cols + 4, ld_bf16=cols + 4, mask=1 - mask, add=1 - mask))
    for rows in (4, 5):          # the packed placement: sample r / 3 of (3 + 5) rows, from row 2 on, + the positional table
        LN_FWD.append(_fwd(f"vec-{cols}x{rows}-packed", rows, cols, GENERAL, 4, ldx=cols + 4, y=1, ldy=cols + 4, period=3, y_row0=2, add=1, beta=1, mask=1,
                           ld_bf16=cols + 12, cols_pad=cols + 8))
LN_FWD.append(_fwd("vec-second-pass", 4 * 8192 + 5, 4, GENERAL, 4, ldx=8, y=1, ldy=8, ld_bf16=8, mask=1, beta=1))
# ---- general, scalar: odd ldx
for ci, cols in enumerate([1, 63, 65, 713, 1023]):
    for ri, rows in enumerate([1, 5]):
        beta, mask = COMBOS[(ci + 2 * ri) % 4]
        LN_FWD.append(_fwd(f"scalar-{cols}x{rows}", rows, cols, GENERAL, 1, ldx=cols + 3 - cols % 2, y=1, ldy=cols + 1, beta=beta, mask=mask, add=ri,
                           cols_pad=up(cols, 8)))
LN_FWD.append(_fwd("scalar-5x1023-packed", 5, 1023, GENERAL, 1, ldx=1025, y=1, ldy=1023, period=3, y_row0=1, add=1, mask=1, ybf=0))
LN_FWD.append(_fwd("scalar-second-pass", 4 * 8192 + 5, 3, GENERAL, 1, ldx=5, y=1, ldy=3, ld_bf16=5, mask=1))
# the dispatch fix: everything the vector form asks of the shapes holds, but y_bf16 sits 2 bytes past an 8-byte boundary
LN_FWD.append(_fwd("vec-shapes-ybf+2-scalar", 5, 260, GENERAL, 1, ldx=264, y=1, ldy=264, ld_bf16=264, ybf_off=2, beta=1))
# the requirement that went: a misaligned add table (read as scalars) keeps the vector form
LN_FWD.append(_fwd("vec-add+4", 5, 260, GENERAL, 4, ldx=264, y=1, ldy=264, ld_bf16=264, add=1, add_off=4))


# ================================================================================================ LayerNorm backward
def _general_cap(rows, knobs):
    return knobs.get(14, 0) or max(256, min(1024, rows // 32))


def _bwd(name, rows, cols, form, width, **kw):
    c = dict(name=name, rows=rows, cols=cols, ldx=cols + 3, ldy=cols + 1, lddx=cols + 2, ld_bf16=cols + 5, x_off=0, gamma_off=0, dxb_off=0,
             mask=0, period=0, y_row0=0, dx=0, dxb=0, dgamma=1, dbeta=0, dxsum=0, knobs={})
    c.update(kw)
    knobs = c["knobs"]
    if form == PARAMS:
        chunks = cdiv(cols, width)
        slabs = max(1, min(1024 // chunks, cdiv(rows, 32)))
        rpb = cdiv(rows, slabs)
        gy = cdiv(rows, rpb)
        c["plan"] = dict(form=form, width=width, grid_x=chunks, grid_y=gy, rows_per_block=rpb, slots=gy, passes=cdiv(rpb, 256 // width))
    else:
        per = 8 if form == TRUNK else 4
        grid = min(cdiv(rows, per), (knobs.get(14, 0) or 256) if form == TRUNK else _general_cap(rows, knobs))
        c["plan"] = dict(form=form, width=width, grid_x=grid, grid_y=1, rows_per_block=per, slots=grid, passes=cdiv(rows, grid * per))
    return c


LN_BWD = []
OUTS2 = [(1, 0), (0, 1), (1, 1)]
# ---- parameter gradients only: a thread per column; 64 / 128 / 256 columns per workgroup, 32 rows or more per slab
for ci, cols in enumerate([1, 64, 65, 128, 129, 256, 257, 713, 1024]):
    for ri, rows in enumerate([1, 31, 33, 97]):
        dgamma, dbeta = OUTS2[(ci + ri) % 3]
        mask, per = COMBOS[(ci + 2 * ri + ci // 4) % 4]
        LN_BWD.append(_bwd(f"params-{cols}x{rows}-g{dgamma}b{dbeta}-m{mask}p{per}", rows, cols, PARAMS, 64 if cols <= 64 else (128 if cols <= 128 else 256),
                           dgamma=dgamma, dbeta=dbeta, mask=mask, period=3 * per, y_row0=2 * per))
# ---- trunk: two rows per wavefront; knob 14 = 2 gives 17 rows a second pass with an odd last row
for ci, cols in enumerate([256, 512, 1024]):
    for ri, rows in enumerate([1, 2, 9, 17]):
        for ki, knobs in enumerate([{}, {14: 2}]):
            dx, dxb = OUTS2[(ci + ri + ki) % 3]
            LN_BWD.append(_bwd(f"trunk-{cols}x{rows}-dx{dx}b{dxb}-k{knobs.get(14, 0)}", rows, cols, TRUNK, cols // 256, ldx=cols + 4, ldy=cols + 4, lddx=cols + 4,
                               ld_bf16=cols + 8, dx=dx, dxb=dxb, knobs=knobs))
# ---- general: vector and scalar, the forward's column lists
for vec, col_list in ((4, [4, 252, 260, 1020, 1024]), (1, [1, 63, 65, 713, 1023])):
    for ci, cols in enumerate(col_list):
        ld = dict(ldx=cols + 4, ldy=cols + 4, lddx=cols + 8, ld_bf16=cols + 4) if vec == 4 else dict(ldx=cols + 3 - cols % 2, ldy=cols + 1, lddx=cols + 2, ld_bf16=cols + 5)
        for ri, rows in enumerate([1, 5, 37]):
            k = (ci + ri) % 3
            tag = f"{'vec' if vec == 4 else 'scalar'}-{cols}x{rows}"
            variants = [
                dict(dx=1, dxb=1, dbeta=1, mask=1),
                dict(dx=1, dbeta=1, period=3, y_row0=1, knobs={14: 2}),
                dict(dxb=1, dbeta=1, dxsum=1, mask=1, period=3, y_row0=2),
            ]
            for v in (variants[k], variants[(k + 1) % 3]):
                LN_BWD.append(_bwd(f"{tag}-" + "".join(f"{a}{b}" for a, b in sorted(v.items()) if a != "knobs") + ("-k2" if "knobs" in v else ""),
                                   rows, cols, GENERAL, vec, **ld, **v))
LN_BWD += [
    _bwd("vec-260x37-dxsum-only", 37, 260, GENERAL, 4, ldx=264, ldy=264, dxsum=1, dgamma=0, mask=1),
    _bwd("scalar-713x5-dxsum-only", 5, 713, GENERAL, 1, dxsum=1, dbeta=1, dgamma=0),
    # the dispatch fix: vector-eligible shapes, dx_bf16 2 bytes past an 8-byte boundary
    _bwd("vec-shapes-dxb+2-scalar", 5, 260, GENERAL, 1, ldx=264, ldy=264, lddx=264, ld_bf16=264, dx=1, dxb=1, dxb_off=2, dbeta=1),
    # knob 12 = 1 at a trunk problem: general, vector
    _bwd("trunk-512x9-knob12", 9, 512, GENERAL, 4, ldx=516, ldy=516, lddx=516, ld_bf16=520, dx=1, dxb=1, knobs={12: 1}),
    # x 4 bytes off a 16-byte boundary at a trunk problem: general, scalar
    _bwd("trunk-512x9-x+4", 9, 512, GENERAL, 1, ldx=516, ldy=516, lddx=516, ld_bf16=520, dx=1, dxb=1, x_off=4),
]

# literal plans (rows, cols, what is asked for) -> numbers, so that the rules above are pinned to something written down
LN_BWD_LITERAL = [
    (dict(rows=97, cols=713, dgamma=1), dict(form=PARAMS, width=256, grid_x=3, grid_y=4, rows_per_block=25, slots=4, passes=25)),
    (dict(rows=4099, cols=74, dgamma=1, dbeta=1, mask=1), dict(form=PARAMS, width=128, grid_x=1, grid_y=129, rows_per_block=32, slots=129, passes=16)),
    (dict(rows=1000, cols=35, dgamma=1), dict(form=PARAMS, width=64, grid_x=1, grid_y=32, rows_per_block=32, slots=32, passes=8)),
    (dict(rows=4099, cols=512, dgamma=1, dx=1, dxb=1, vec_ld=1), dict(form=TRUNK, width=2, grid_x=256, grid_y=1, rows_per_block=8, slots=256, passes=3)),
    (dict(rows=1000, cols=512, dgamma=1, dx=1, dxb=1, vec_ld=1), dict(form=TRUNK, width=2, grid_x=125, grid_y=1, rows_per_block=8, slots=125, passes=1)),
    (dict(rows=330, cols=74, dgamma=1, dbeta=1, dxsum=1, dx=1, dxb=1, mask=1, period=30), dict(form=GENERAL, width=1, grid_x=83, grid_y=1, rows_per_block=4,
                                                                                              slots=83, passes=1)),
    (dict(rows=48000, cols=512, dgamma=1, dbeta=1, dx=1, vec_ld=1), dict(form=GENERAL, width=4, grid_x=1024, grid_y=1, rows_per_block=4, slots=1024, passes=12)),
]
LN_FWD_LITERAL = [
    (dict(rows=48000, cols=74, ybf=1, beta=1, mask=1, cols_pad=80), dict(form=NARROW, width=0, grid_x=3000, passes=1)),
    (dict(rows=16 * 4096 + 17, cols=1, ybf=1), dict(form=NARROW, width=0, grid_x=4096, passes=2)),
    (dict(rows=4099, cols=512, ybf=1, vec_ld=1), dict(form=TRUNK, width=2, grid_x=513, passes=1)),
    (dict(rows=32773, cols=4, ybf=1, y=1, vec_ld=1), dict(form=GENERAL, width=4, grid_x=8192, passes=2)),
    (dict(rows=9, cols=257, ybf=1), dict(form=GENERAL, width=1, grid_x=3, passes=1)),
]

# ================================================================================================ the other kernels' shapes
CAST_PAD = [          # rows, cols, lds, rows_pad, cols_pad, ldd, transpose
    (1, 1, 3, 1, 1, 4, 0), (3, 5, 7, 64, 64, 72, 0), (65, 63, 63, 128, 72, 75, 0), (130, 70, 71, 72, 136, 137, 1),
]
GEGLU = [(1, 8), (3, 1416), (4099, 2056)]          # (rows, ip); the last exceeds 4096 x 256 chunks of 8: a second pass of the grid-stride loop
SQNORM_N = [1, 2, 3, 4, 5, 1023, 1024, 1027, 256 * 1024 * 4 + 3]
ADAMW_N = [1, 255, 257, 4096 * 256 + 3]
FLAG_N = [0, 1, 3, 4, 5, 1027]
