"""The shapes of the GEMM tests, in one place: tests/test_kernels_gpu.py runs them on the GPU and tests/test_gemm_plan_cpu.py
asks the library which kernel each of them reaches (mca_dbg_plan_gemm_*), so that what a shape is in the list for is an
asserted fact and not a comment.  A "call" below is one entry-point call as a plain dict: the form the recorded dispatch table
(tests/golden/gemm_dispatch.json) and the plan helper of the CPU test share."""

# (M, N, K) of test_gemm_nt
NT = [(300, 200, 128), (1000, 1536, 512), (129, 2816, 512), (16, 512, 512), (4060, 512, 1408),
      (4100, 1536, 320), (2600, 2816, 512),          # persistent kernels, grouped column tiles
      (17920, 1024, 192), (17700, 1024, 256),        # 280 tiles of 256 x 256 on 256 CUs: second tile per workgroup, shortest k-loops
      (2100, 384, 320)]                              # N % 256 != 0: the 256 x 128 persistent kernel with bf16 output and no bias
NT_LNRES = [(2304, 512, 512), (4100, 512, 1408), (2100, 256, 576)]
# (R, N, K, lda, ldb) of test_gemm_tn_acc
TN_ACC = [(1000, 512, 512, 512, 512), (777, 1365, 512, 2816, 512), (2048, 512, 1365, 512, 1408),
          (16, 512, 512, 512, 512), (500, 128, 74, 128, 128), (5000, 1024, 512, 1536, 512)]
# (R, [(N, K, lda, ldb)]) of test_gemm_tn_acc_group
TN_GROUP = [
    (8192, [(1536, 512, 1536, 512), (1365, 512, 2816, 512), (1365, 512, 2816, 512), (512, 1365, 512, 1408)]),   # a layer's four
    # a layer's five (with the out-projection): 52 tiles = 4 whole splits + 48 spans that end one tile's rows and begin the next's
    (8200, [(1536, 512, 1536, 512), (1365, 512, 2816, 512), (1365, 512, 2816, 512), (512, 1365, 512, 1408), (512, 512, 512, 512)]),
    # ... and the pooling key/value projection on top (the top layer's launch), at the b = 8 row count
    (20304, [(1536, 512, 1536, 512), (1365, 512, 2816, 512), (1365, 512, 2816, 512), (512, 1365, 512, 1408), (512, 512, 512, 512),
             (1024, 512, 1024, 512)]),
    (4100, [(512, 512, 512, 512), (300, 700, 304, 704), (1024, 256, 1024, 256), (256, 256, 256, 256), (515, 260, 520, 264)]),
    (5000, [(512, 512, 512, 512), (100, 512, 104, 512)]),          # a member the grouped kernel does not take -> single launches
    (300, [(512, 512, 512, 512), (512, 256, 512, 256)]),           # too few rows -> single launches
]
TN_GROUP_UNIFORM_SPLITS = 3          # knob 3 of the second pass of test_gemm_tn_acc_group
# (rows, ip, D)
GEGLU_FWD = [(500, 384, 128), (4100, 384, 128), (4100, 384, 512), (2304, 448, 320), (2100, 1408, 512),
             (8200, 1408, 192), (8200, 1408, 512)]          # 363 tiles: a second tile per workgroup
GEGLU_BWD = [(500, 384, 128), (4100, 384, 128), (4100, 384, 512), (2304, 640, 320), (2100, 1408, 512),
             (41100, 384, 128), (41100, 384, 512)]          # >= 40,960 rows: the 256-row kernels

# the step's GEMMs: tokens per sample of the CMU and LONG workloads (FusionStructure.n_tokens), model width, padded inner width
CMU_TOKENS, LONG_TOKENS, D, IP, IP_RAW = 2538, 6088, 512, 1408, 1365
STEP_ROWS = {"cmu_b2": 2 * CMU_TOKENS, "cmu_b8": 8 * CMU_TOKENS, "cmu_b32": 32 * CMU_TOKENS,
             "long_b16": 16 * LONG_TOKENS, "long_b128": 128 * LONG_TOKENS}
LAYER_GRADS = [(3 * D, D), (IP_RAW, D), (IP_RAW, D), (D, IP_RAW), (D, D), (2 * D, D)]          # (N, K): qkv, ff1 halves, ff2, out, pooling kv


def nt(M, N, K, out_bf16=0, res=0, bias=0, c_off=0, ldc=None, res_off=0, ldres=None, bias_off=0):
    """res: 0 none, 1 per row, 2 periodic.  *_off: byte offset of the pointer from a 256-byte boundary (alignment cases)."""
    return dict(entry="nt", M=M, N=N, K=K, out_bf16=out_bf16, res=res, bias=bias, c_off=c_off, ldc=N if ldc is None else ldc,
                res_off=res_off, ldres=N if ldres is None else ldres, bias_off=bias_off)


def fused(entry, M, N, K):
    """entry: lnres | geglu_fwd | geglu_bwd (N = ip)"""
    return dict(entry=entry, M=M, N=N, K=K)


def tn(R, N, K):
    return dict(entry="tn", R=R, N=N, K=K)


def tn_group(R, members):
    return dict(entry="tn_group", R=R, members=[[m[0], m[1]] for m in members])


def gemm_nt_test_calls(M, N, K):
    """the calls of one test_gemm_nt case, in its order"""
    calls = [nt(M, N, K), nt(M, N, K, res=1, bias=1), nt(M, N, K, out_bf16=1),
             nt(M, N, K, bias=1), nt(M, N, K, out_bf16=1, bias=1), nt(M, N, K, out_bf16=1, res=1, bias=1)]
    if M % 16 == 0:
        calls += [nt(M, N, K, res=2), nt(M, N, K, out_bf16=1, res=2)]
    return calls


def suite_calls():
    """every GEMM entry-point call the GPU tests of these lists make with all knobs 0"""
    calls = [c for s in NT for c in gemm_nt_test_calls(*s)]
    calls += [fused("lnres", *s) for s in NT_LNRES]
    calls += [tn(R, N, K) for R, N, K, _, _ in TN_ACC]
    calls += [tn_group(R, ms) for R, ms in TN_GROUP]
    calls += [fused("geglu_fwd", *s) for s in GEGLU_FWD] + [fused("geglu_bwd", *s) for s in GEGLU_BWD]
    return calls


def step_calls(T):
    """the GEMM launches of one fusion layer's forward and backward over T token rows (tools/bench_step_gemms.py), and its weight
    gradients alone, as a layer's four / five and as the top layer's six"""
    calls = [nt(T, 3 * D, D, out_bf16=1), nt(T, D, 2 * IP, res=1), nt(T, D, 3 * D, res=1), nt(T, D, D, out_bf16=1),
             fused("geglu_bwd", T, IP, D), fused("geglu_fwd", T, IP, D), fused("lnres", T, D, D), fused("lnres", T, D, IP)]
    calls += [tn(T, N, K) for N, K in LAYER_GRADS]
    calls += [tn_group(T, LAYER_GRADS[:n]) for n in (4, 5, 6)]
    return calls
