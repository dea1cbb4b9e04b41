"""The listed cases of the token-table edge tests (tests/test_token_edges_gpu.py) for csrc/embedding.hip, each with the grid and
the number of loop passes it reaches in each of its launches; tests/test_token_edges_cpu.py asserts them without a GPU.
Nothing here is drawn: the lists are crosses of the sizes at which the kernels change path, pruned by the index arithmetic of the
loops below to the combinations that reach a distinct path.

The three constants the grids follow from (csrc/embedding.hip): wave_grid caps every grid at GRID_CAP workgroups of WAVES
wavefronts; embedding_renorm_marked_kernel takes RENORM_CHUNK markers per wavefront; embedding_mark_kernel a token per thread."""
GRID_CAP, WAVES, RENORM_CHUNK = 2048, 4, 16
LANES, BLOCK, SORT_TILE = 64, 256, 256
EXTRA = 3                     # rows between two samples of a packed placement: bstride = (period + 3) ld
OOB_BIT, FLAG_PRESET = 4, 2   # the bit a lookup ORs into the flag word, and the other bit the word holds already
COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]          # (add, accumulate)


def cdiv(a, b):
    return (a + b - 1) // b


def wave_grid(waves):
    return max(1, min(cdiv(waves, WAVES), GRID_CAP))


def lookup_plan(vocab, cols, tokens):
    """(grid, passes of the grid-stride loop) of the three launches; lane_passes: trips of the renormalisation's 64-column loop and
    of the gather's 64-float4 loop"""
    gm, gr, gg = wave_grid(cdiv(tokens, LANES)), wave_grid(cdiv(vocab, RENORM_CHUNK)), wave_grid(tokens)
    return dict(mark=(gm, cdiv(tokens, gm * BLOCK)), renorm=(gr, cdiv(vocab, gr * WAVES * RENORM_CHUNK)), gather=(gg, cdiv(tokens, gg * WAVES)),
                lane_passes=(cdiv(cols, LANES), cdiv(cols // 4, LANES)))


def grad_plan(vocab, cols, tokens):
    """scatter: (grid, passes); sort: (grid, LDS tiles each thread walks); sum: (items, grid, passes); chunks of 64 columns and
    whether the last one is partial (the `c < cols` guard)"""
    gs = wave_grid(tokens)
    chunks = cdiv(cols, LANES)
    items = tokens * chunks
    gi = wave_grid(items)
    return dict(scatter=(gs, cdiv(tokens, gs * WAVES)), sort=(cdiv(tokens, SORT_TILE), cdiv(tokens, SORT_TILE)), sum=(items, gi, cdiv(items, gi * WAVES)),
                chunks=chunks, partial_chunk=int(cols % LANES != 0))


# ================================================================================================ lookup
L_COLS = [4, 60, 64, 68, 256, 260, 1024]
L_VOCAB = [1, 15, 16, 17, 33]
L_TOKENS = [1, 3, 4, 5, 10]
L_PATTERNS = ["same", "distinct", "ends", "oob", "mixed"]
MAX_NORMS = [1.0, 0.5, 2.5]          # their squares are exact in fp32


def _lookup(name, vocab, cols, tokens, period, pattern, add, acc, **kw):
    c = dict(name=name, vocab=vocab, cols=cols, tokens=tokens, period=period, pattern=pattern, add=add, acc=acc, ldd=cols, idx_bytes=8, max_norm=1.0,
             cls0=0, flag=1, second=None)
    c.update(kw)
    c["oob"] = int(pattern in ("oob", "oob-tail"))
    c["plan"] = lookup_plan(vocab, cols, tokens)
    assert all(c["plan"][k] == v for k, v in c.pop("pin", {}).items()), name          # the numbers a listed case is there for
    return c


LOOKUP = []
for ci, cols in enumerate(L_COLS):
    for ti, tokens in enumerate(L_TOKENS):
        k = ci + ti
        add, acc = COMBOS[(ci + 3 * ti) % 4]
        vocab = L_VOCAB[(2 * ci + ti) % 5]
        pattern = L_PATTERNS[(ci + 2 * ti) % 5]
        period = (1, 7, tokens)[k % 3]
        LOOKUP.append(_lookup(f"{cols}x{tokens}-v{vocab}-p{period}-{pattern}-a{add}c{acc}", vocab, cols, tokens, period, pattern, add, acc,
                              ldd=cols + 4 * (k % 2), idx_bytes=(8, 4)[(ci + ti // 2) % 2], max_norm=MAX_NORMS[k % 3], cls0=k % 5))
# an index out of range under each of the four (add, accumulate) combinations (each writes something else), a partial last group
for add, acc in COMBOS:
    for ib in (8, 4):
        LOOKUP.append(_lookup(f"oob-68x10-a{add}c{acc}-i{ib * 8}", 17, 68, 10, 7, "oob", add, acc, ldd=72, idx_bytes=ib, max_norm=MAX_NORMS[(add + 2 * acc) % 3]))
LOOKUP += [
    _lookup("oob-flag-null", 17, 64, 10, 7, "oob", 1, 0, ldd=68, flag=0),
    _lookup("every-class-named", 33, 260, 33, 33, "distinct", 1, 1, ldd=264, idx_bytes=4),          # 33 tokens: every row once, all five norm classes
    _lookup("every-class-named-2.5", 33, 64, 33, 7, "distinct", 0, 0, idx_bytes=4, max_norm=2.5, cls0=2),
    _lookup("every-class-named-0.5", 33, 1024, 33, 7, "distinct", 0, 1, ldd=1028, max_norm=0.5, cls0=4),
    # the second passes, at cols = 4
    _lookup("gather-second-pass", 33, 4, GRID_CAP * WAVES + 5, 7, "mixed", 1, 1, ldd=8, idx_bytes=4, pin=dict(gather=(2048, 2), mark=(33, 1))),
    _lookup("same-row-8197", 17, 4, GRID_CAP * WAVES + 5, GRID_CAP * WAVES + 5, "same", 0, 0, max_norm=2.5, pin=dict(gather=(2048, 2))),
    _lookup("renorm-second-pass", GRID_CAP * WAVES * RENORM_CHUNK + 17, 4, 10, 7, "straddle", 1, 0, ldd=8, max_norm=0.5, pin=dict(renorm=(2048, 2))),
    _lookup("mark-second-pass", 33, 4, GRID_CAP * BLOCK + 5, GRID_CAP * BLOCK + 5, "oob-tail", 0, 0, idx_bytes=4, pin=dict(mark=(2048, 2), gather=(2048, 65))),
    # two lookups back to back on one marker and one table, as a training run does: the second names other rows
    _lookup("two-lookups", 33, 64, 10, 7, "mixed", 1, 0, ldd=68, second="second"),
]

LOOKUP_LITERAL = [          # (vocab, cols, tokens) -> the numbers, written down
    ((33, 64, 10), dict(mark=(1, 1), renorm=(1, 1), gather=(3, 1), lane_passes=(1, 1))),
    ((17, 68, 10), dict(mark=(1, 1), renorm=(1, 1), gather=(3, 1), lane_passes=(2, 1))),
    ((33, 256, 5), dict(mark=(1, 1), renorm=(1, 1), gather=(2, 1), lane_passes=(4, 1))),
    ((33, 260, 33), dict(mark=(1, 1), renorm=(1, 1), gather=(9, 1), lane_passes=(5, 2))),
    ((33, 1024, 33), dict(mark=(1, 1), renorm=(1, 1), gather=(9, 1), lane_passes=(16, 4))),
    ((33, 4, 8197), dict(mark=(33, 1), renorm=(1, 1), gather=(2048, 2), lane_passes=(1, 1))),
    ((131089, 4, 10), dict(mark=(1, 1), renorm=(2048, 2), gather=(3, 1), lane_passes=(1, 1))),
    ((33, 4, 524293), dict(mark=(2048, 2), renorm=(1, 1), gather=(2048, 65), lane_passes=(1, 1))),
    ((131072, 4, 8192), dict(mark=(32, 1), renorm=(2048, 1), gather=(2048, 1), lane_passes=(1, 1))),          # the last sizes of one pass
    ((33, 4, 524288), dict(mark=(2048, 1), renorm=(1, 1), gather=(2048, 64), lane_passes=(1, 1))),
]


# ================================================================================================ table gradient
G_COLS = [1, 63, 64, 65, 128, 129, 1024]
G_TOKENS = [1, 255, 256, 257, 513]
G_PATTERNS = ["one", "cyclic", "descending", "allpad", "alloob", "mixed"]
G_PADS = [0, 5, -1, "vocab"]


def _grad(name, vocab, cols, tokens, period, pattern, pad, **kw):
    c = dict(name=name, vocab=vocab, cols=cols, tokens=tokens, period=period, pattern=pattern, padding_idx=vocab if pad == "vocab" else pad, ldy=cols)
    c.update(kw)
    c["plan"] = grad_plan(vocab, cols, tokens)
    assert all(c["plan"][k] == v for k, v in c.pop("pin", {}).items()), name          # the numbers a listed case is there for
    return c


GRAD = []
for ci, cols in enumerate(G_COLS):
    for ti, tokens in enumerate(G_TOKENS):
        k = ci + ti
        vocab = 1 if k % 5 == 4 else 37
        pattern = G_PATTERNS[(ci + 2 * ti) % 6]
        pad = G_PADS[(ci + 3 * ti) % 4]
        period = (1, 7, tokens)[k % 3]
        GRAD.append(_grad(f"{cols}x{tokens}-v{vocab}-p{period}-{pattern}-pad{pad}", vocab, cols, tokens, period, pattern, pad, ldy=cols + 3 * (k % 2)))
GRAD += [
    # every token another row, and strictly descending rows, across the 256 tile: a table of more rows than tokens
    _grad("distinct-257", 300, 64, 257, 7, "distinct", 0, ldy=67),
    _grad("strictly-descending-257", 300, 65, 257, 257, "strict-descending", 5),
    # each padding_idx form with the padding row named among others, a partial last group
    *[_grad(f"mixed-129x257-pad{p}", 37, 129, 257, 7, "mixed", p, ldy=132) for p in G_PADS],
    *[_grad(f"v1-64x257-pad{p}", 1, 64, 257, 7, "one", p, ldy=67) for p in G_PADS],
    _grad("sum-second-pass", 37, 1024, 600, 150, "three-rows", 0, ldy=1027, pin=dict(sum=(9600, 2048, 2), scatter=(150, 1), sort=(3, 3))),          # 9600 (place, chunk) items
    _grad("atomic-second-pass", 37, 4, GRID_CAP * WAVES + 5, 7, "one", 5, ldy=7, pin=dict(scatter=(2048, 2), sort=(33, 33), sum=(8197, 2048, 2))),     # 8197 tokens, all one row: sums up to 8197 x 4 + 8
    _grad("atomic-second-pass-mixed", 37, 4, GRID_CAP * WAVES + 5, GRID_CAP * WAVES + 5, "mixed", -1, pin=dict(scatter=(2048, 2))),
]

GRAD_LITERAL = [          # (vocab, cols, tokens) -> the numbers, written down
    ((37, 1, 1), dict(scatter=(1, 1), sort=(1, 1), sum=(1, 1, 1), chunks=1, partial_chunk=1)),
    ((37, 64, 256), dict(scatter=(64, 1), sort=(1, 1), sum=(256, 64, 1), chunks=1, partial_chunk=0)),
    ((37, 65, 257), dict(scatter=(65, 1), sort=(2, 2), sum=(514, 129, 1), chunks=2, partial_chunk=1)),
    ((1, 129, 513), dict(scatter=(129, 1), sort=(3, 3), sum=(1539, 385, 1), chunks=3, partial_chunk=1)),
    ((37, 1024, 513), dict(scatter=(129, 1), sort=(3, 3), sum=(8208, 2048, 2), chunks=16, partial_chunk=0)),
    ((37, 1024, 600), dict(scatter=(150, 1), sort=(3, 3), sum=(9600, 2048, 2), chunks=16, partial_chunk=0)),
    ((37, 1024, 512), dict(scatter=(128, 1), sort=(2, 2), sum=(8192, 2048, 1), chunks=16, partial_chunk=0)),
    ((37, 4, 8197), dict(scatter=(2048, 2), sort=(33, 33), sum=(8197, 2048, 2), chunks=1, partial_chunk=1)),
    ((37, 4, 8192), dict(scatter=(2048, 1), sort=(32, 32), sum=(8192, 2048, 1), chunks=1, partial_chunk=1)),
]
