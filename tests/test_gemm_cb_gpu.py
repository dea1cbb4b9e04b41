"""mca_gemm_nt_cb (the 256 x 256 persistent kernel with the column-blocked store) against mca_gemm_nt on the same operands: the
slabs [N / 64][M][64], un-blocked, equal the row-major bf16 output BIT FOR BIT at every element, and no byte outside rows
0 .. M - 1 of a slab changes.  The slabs lie (M + 5) * 64 elements apart inside one sentinel-filled allocation, so the five rows
between two slabs, and guard rows in front of the first and behind the last, catch a store that misses its slab.  Random bf16
operands (not the integer ones of the edge tests: the comparison is between two kernels with the same k-loop, not with fp64)."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 8 * 64          # sentinel elements in front of slab 0 and behind the last slab's frame
SENTINEL = -1           # int16 0xFFFF: a bf16 NaN, so an element nobody stored fails the comparison too


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def operands(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = (torch.randn(M, K, device="cuda", generator=g)).bfloat16()
    B = (torch.randn(N, K, device="cuda", generator=g) * 0.25).bfloat16()
    return A, B


def run_cb(H, A, B, M, N, K):
    """-> (the whole allocation as int16, the [N / 64] x [M + 5] x [64] view of its slabs, frame rows included)"""
    cbs, nb = (M + 5) * 64, N // 64
    buf = torch.full((GUARD + nb * cbs + GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
    c = buf[GUARD:]
    assert c.data_ptr() % 16 == 0
    H.call("mca_gemm_nt_cb", A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), c.data_ptr(), cbs, M, N, K, H.stream_ptr())
    torch.cuda.synchronize()
    return buf, buf[GUARD:GUARD + nb * cbs].view(nb, M + 5, 64)


@pytest.mark.parametrize("M,N,K", [(2085, 256, 192), (2085, 256, 512), (2085, 512, 192), (2085, 512, 512), (2085, 1536, 192),
                                   (2085, 1536, 512), (11520, 1536, 192)])
def test_cb_store_matches_the_row_major_store_bit_for_bit(H, M, N, K):
    """M = 2085: the last row tile has 37 rows; M = 11,520 x N = 1536: 270 tiles, more than the CUs, so a workgroup walks a second
    tile with the first one's stores in flight"""
    A, B = operands(M, N, K, 1000 + N + K)
    ref = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    H.call("mca_gemm_nt", A.data_ptr(), K, B.data_ptr(), K, ref.data_ptr(), N, 1, None, None, 0, 0, M, N, K, H.stream_ptr())
    buf, slabs = run_cb(H, A, B, M, N, K)
    assert torch.isfinite(ref.float()).all() and float(ref.float().abs().max()) > 1.0
    got = slabs[:, :M].permute(1, 0, 2).reshape(M, N)          # un-block: column n = slab n // 64, position n % 64
    bad = got != ref.view(torch.int16)
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} elements differ; first (row, column): {bad.nonzero()[:8].tolist()}"
    # the frame: rows M .. M + 4 of every slab, and the guards at both ends
    assert bool((slabs[:, M:] == SENTINEL).all()), "a store landed between two slabs"
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), "a store landed outside the slabs"


@pytest.mark.parametrize("what,M,N,K,cbs,off,rc", [
    ("M < 2048", 2000, 512, 512, None, 0, -3), ("N % 256", 2085, 320, 512, None, 0, -3), ("K < 192", 2085, 512, 128, None, 0, -3),
    ("cbs % 8", 2085, 512, 512, 2085 * 64 + 4, 0, -3), ("cbs < M * 64", 2085, 512, 512, 2084 * 64, 0, -3),
    ("C misaligned", 2085, 512, 512, None, 4, -3), ("K % 32", 2085, 512, 208, None, 0, -2)])
def test_cb_entry_returns_its_error_code_and_stores_nothing(H, what, M, N, K, cbs, off, rc):
    A, B = operands(M, N, max(K, 32), 5)
    cbs = (M + 5) * 64 if cbs is None else cbs
    buf = torch.full((GUARD + (N // 64 + 1) * (M + 5) * 64,), SENTINEL, dtype=torch.int16, device="cuda")
    got = H.lib().mca_gemm_nt_cb(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), buf.data_ptr() + 2 * (GUARD + off), cbs, M, N, K,
                                 H.stream_ptr())
    torch.cuda.synchronize()
    assert got == rc, what
    assert bool((buf == SENTINEL).all())


def test_cb_entry_follows_the_knobs(H):
    """knobs 1, 7 and 10 take mca_gemm_nt off the 256 x 256 kernel: the blocked store does not exist there, the entry refuses"""
    M, N, K = 2085, 512, 192
    A, B = operands(M, N, K, 6)
    buf = torch.full((N // 64 * M * 64,), SENTINEL, dtype=torch.int16, device="cuda")
    for knob, value in ((1, 1), (7, 1), (10, 1)):
        with H.knobs(**{f"k{knob}": value}):
            assert H.lib().mca_gemm_nt_cb(A.data_ptr(), K, B.data_ptr(), K, buf.data_ptr(), M * 64, M, N, K, H.stream_ptr()) == -3
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
