"""The listed cases of the top-k retrieval tests (tests/test_retrieval_gpu.py; tests/test_retrieval_cpu.py): the raw entry point
mca_cosine_topk_f32 at the sizes where the 64 x 64 tile core, its 16-wide K staging, the k-entry lists and the 16-tile (1024-target)
chunks change path.  Nothing here is drawn: the list is written out by the loop below, a covering subset of the sizes, not their
product.  Every operand of a case has a leading dimension of its columns + 3 (eval_cases.PAD)."""
from eval_cases import KC, PAD, TILE, cdiv          # noqa: F401

TOPK_TILES_PER_CHUNK = 16
CHUNK = TILE * TOPK_TILES_PER_CHUNK          # 1024 targets per workgroup
TOPK_MAX = 64

NQS = (1, 63, 64, 65)
DS = (1, 16, 17, 96)
KS = (1, 2, 10, 63, 64)
NTS = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)

# options: bit 0 qidx (a gather, descending with a repeat), bit 1 tvalid, bit 2 exclude; every case number n takes options n % 8
TOPK = []
for i, nt in enumerate(NTS):
    for j, nq in enumerate(NQS):
        n = 4 * i + j
        d, k, opt = DS[(i + j) % 4], KS[n % 5], n % 8
        TOPK.append(dict(name=f"topk-q{nq}t{nt}d{d}k{k}-o{opt}", nq=nq, nt=nt, d=d, k=k, qidx=opt & 1, tvalid=(opt >> 1) & 1, exclude=(opt >> 2) & 1))


def chunks(nt):
    return cdiv(cdiv(nt, TILE), TOPK_TILES_PER_CHUNK)


def workspace_bytes(nq, nt, k):
    return chunks(nt) * nq * k * 8
