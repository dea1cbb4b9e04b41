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


# ------------------------------------------------------------------------------------------------------------------------
# Edge cases of tests/test_gemm_edges_gpu.py: tails, strides, misaligned pointers, shortest k-loops.  They are NOT part of
# suite_calls() (the recorded dispatch table covers that list and does not change); test_gemm_plan_cpu.py asserts the kernel
# and the property each one is listed for (test_gemm_edge_shapes_reach_what_they_are_listed_for).
# ------------------------------------------------------------------------------------------------------------------------
NT_FORMS = [(0, 0, 0), (0, 1, 1), (1, 0, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1)]          # (out_bf16, res, bias): the six of test_gemm_nt
NT_FORMS_PERIODIC = [(0, 2, 0), (1, 2, 0)]                                             # ... and its two with M % 16 == 0
F32_RES = [(0, 1, 0), (0, 1, 1)]
PERSIST_FORMS = [(1, 0, 0), (1, 0, 1), (0, 0, 0), (0, 0, 1)]                           # modes 0 and 1, without and with bias


def edge_nt(name, M, N, K, forms=None, lda=None, ldb=None, ldc=None, ldres=None, c_off=0, res_off=0, bias_off=0):
    """One mca_gemm_nt edge case.  c_off is in ELEMENTS of the output (4 bytes fp32, 2 bytes bf16), res_off / bias_off in bytes."""
    if forms is None:
        forms = NT_FORMS + (NT_FORMS_PERIODIC if M % 16 == 0 else [])
    return dict(name=name, M=M, N=N, K=K, forms=forms, lda=lda or K, ldb=ldb or K, ldc=ldc or N, ldres=ldres or N,
                c_off=c_off, res_off=res_off, bias_off=bias_off)


EDGE_NT = [
    edge_nt("glds_tails", 130, 70, 64),                    # 128 x 128 kernel: row tail of 2, partial 4- and 8-element pieces, one k-step,
    edge_nt("glds_tails_periodic", 144, 70, 64),           # ... row pointers 16-byte aligned only every second / fourth row
    edge_nt("glds_strides", 130, 136, 128, lda=136, ldb=144, ldc=152, ldres=144),          # a full piece inside a partial column tile
    edge_nt("nt256_k64", 2050, 136, 64),                   # 3-stage kernel, k-loop shorter than its prefetch distance, N and row tails
    edge_nt("nt256_k128", 2050, 136, 128),
    edge_nt("nt256_k64_periodic", 2064, 136, 64),
    edge_nt("nt256_c_misaligned", 2050, 256, 128, ldc=264, c_off=1),                          # the scalar store path
    edge_nt("nt256_res_bias_misaligned", 2050, 256, 128, ldc=264, res_off=4, bias_off=4),     # the unaligned residual path
    edge_nt("nt256_prefetch_strided", 2050, 128, 512, forms=F32_RES, ldc=132, ldres=132),
    edge_nt("nt256_prefetch_refused", 2050, 128, 512, forms=F32_RES, res_off=4),              # misaligned residual: no prefetch
    edge_nt("persist_9_tiles", 2050, 128, 320, forms=PERSIST_FORMS, ldc=136),
    edge_nt("persist_261_tiles", 2050, 3712, 320, forms=PERSIST_FORMS, ldc=3720),             # a second tile per workgroup, strided C
    edge_nt("persist256_261_tiles", 2050, 7424, 192, forms=[(1, 0, 0)], ldc=7432),            # its shortest k-loop
    edge_nt("encoder_projection", 2050, 512, 64, forms=[(0, 0, 1)]),                          # kp = 64, rows >= 2048: production
]
EDGE_NT_LNRES = [(2050, 128, 512, 132, 132)]          # (M, N, K, ldc, ldx): the smallest shape the entry point accepts
# (rows, ip, D); the fused cases run with ldh = 2 * ip + 8 and ldg = ip + 8, the unfused pair takes packed rows only
EDGE_GEGLU_FWD = [(2050, 128, 192), (2050, 3712, 192), (2050, 192, 320), (2050, 72, 64)]
EDGE_GEGLU_BWD = [(130, 72, 64), (40962, 72, 64), (40962, 128, 320), (40962, 256, 320)]          # all with ldh = 2 * ip + 8
# (R, N, K, lda, ldb); C has ldc = K + 4
EDGE_TN = [(70, 72, 40, 80, 48), (300, 136, 72, 144, 80), (4100, 520, 72, 528, 80), (4100, 776, 520, 784, 528)]
# (R, [(N, K, lda, ldb)]): 26 tiles = 2 whole splits + 157 span workgroups of the minimum span (128 rows)
EDGE_TN_GROUP = [(4100, [(776, 520, 784, 528), (520, 264, 528, 272), (264, 776, 272, 784)])]


def edge_nt_calls(case):
    """the plan-level calls of one EDGE_NT case, in the order of its forms"""
    out = []
    for ob, res, bias in case["forms"]:
        out.append(nt(case["M"], case["N"], case["K"], out_bf16=ob, res=res, bias=bias, c_off=case["c_off"] * (2 if ob else 4), ldc=case["ldc"],
                      res_off=case["res_off"] if res else 0, ldres=case["ldres"], bias_off=case["bias_off"] if bias else 0))
    return out


def edge_calls():
    """every GEMM entry-point call of the edge tests with all knobs 0"""
    calls = [c for case in EDGE_NT for c in edge_nt_calls(case)]
    calls += [fused("lnres", M, N, K) for M, N, K, _, _ in EDGE_NT_LNRES]
    calls += [fused("geglu_fwd", *s) for s in EDGE_GEGLU_FWD] + [fused("geglu_bwd", *s) for s in EDGE_GEGLU_BWD]
    calls += [tn(R, N, K) for R, N, K, _, _ in EDGE_TN]
    calls += [tn_group(R, ms) for R, ms in EDGE_TN_GROUP]
    return calls
