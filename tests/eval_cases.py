"""The listed cases of the evaluation-kernel edge tests (tests/test_eval_edges_gpu.py; tests/test_eval_edges_cpu.py): the raw entry
points of csrc/evaluate.hip at the sizes where the 64 x 64 tile core, its 16-wide K staging, the 16-tile rank chunks, the 128-row
weight-gradient chunks and the 64-lane row kernels change path.  Nothing here is drawn: the lists are written out by the loops below.
Every operand of a case has a leading dimension of its columns + 3."""
TILE, KC, RANK_TILES_PER_CHUNK, PROBE_ROWS_PER_CHUNK = 64, 16, 16, 128
PAD = 3


def cdiv(a, b):
    return (a + b - 1) // b


NORMALIZE = [dict(name=f"normalize-n{n}d{d}", n=n, d=d) for n in (1, 3, 4, 5) for d in (1, 63, 64, 65, 130)]

# qidx: None, or a gather that is out of order and repeats (forced where nq > nt: without it query r's target is target r)
RANK = []
for i, (nq, nt, d) in enumerate((nq, nt, d) for nq in (1, 63, 64, 65) for nt in (1, 63, 65, 1024, 1025) for d in (1, 15, 16, 17, 96)):
    gather = nq > nt or i % 2 == 1
    RANK.append(dict(name=f"rank-q{nq}t{nt}d{d}-{'gather' if gather else 'plain'}", nq=nq, nt=nt, d=d, gather=gather))

PAIR = [dict(name=f"pair-n{n}d{d}", n=n, d=d) for n in (0, 1, 2, 63, 64, 65, 129) for d in (1, 16, 17)]

# (act, p, bias, gather): act 0 none, 1 ReLU, 2 dropout then ReLU; p = 0.25 is the one form whose scale is not a power of two
NT_FORMS = [(0, 0.0, 0, 0), (1, 0.0, 1, 1), (2, 0.0, 1, 0), (2, 0.5, 1, 1), (2, 1.0, 1, 0), (2, 0.25, 1, 1), (0, 0.0, 1, 1), (1, 0.0, 0, 0)]
PROBE_NT = []
for i, (M, N, K) in enumerate((M, N, K) for M in (1, 64, 65) for N in (1, 63, 64, 65, 130) for K in (1, 15, 16, 17, 96)):
    for act, p, bias, gather in (NT_FORMS[i % 8], NT_FORMS[(i + 3) % 8], NT_FORMS[(i + 5) % 8]):
        PROBE_NT.append(dict(name=f"nt-M{M}N{N}K{K}-act{act}p{p}b{bias}g{gather}", M=M, N=N, K=K, act=act, p=p, bias=bias, gather=gather))

L1, MSE, BCE = 0, 1, 2
# flags: bit 0 dz, bit 1 da, bit 2 aidx, bit 3 yidx
PROBE_HEAD = []
for i, (K, L, B) in enumerate((K, L, B) for K in (1, 63, 64, 65, 1023, 1024) for L in (1, 2, 63, 64) for B in (1, 3, 4, 5)):
    for loss, flags in ((i % 3, (5 * i + 3) % 16), ((i + 1) % 3, (5 * i + 12) % 16)):
        PROBE_HEAD.append(dict(name=f"head-K{K}L{L}B{B}-loss{loss}f{flags}", K=K, L=L, B=B, loss=loss, dz=flags & 1, da=(flags >> 1) & 1, aidx=(flags >> 2) & 1,
                               yidx=(flags >> 3) & 1))

PROBE_TN = []
for i, (R, N, K) in enumerate((R, N, K) for R in (1, 127, 128, 129, 300) for N in (1, 64, 65) for K in (1, 62, 63, 64, 127)):
    PROBE_TN.append(dict(name=f"tn-R{R}N{N}K{K}-{'gather' if i % 2 else 'plain'}", R=R, N=N, K=K, gather=i % 2))

LOSS_ACCUM = [1, 63, 64, 65, 200]
