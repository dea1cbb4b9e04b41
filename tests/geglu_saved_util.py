"""Helpers of the saved-factor GEGLU tests (tests/test_geglu_saved_cpu.py, tests/test_geglu_saved_gpu.py): the float64
factors s = [gelu(gate) | a * gelu'(gate)] of a given h = [a | gate], and the element-wise bounds.  Plain functions on any
device, no fixtures.

The bound on s.  A kernel computes a factor v in fp32 and rounds it ONCE to bf16.  With E the error of the fp32 value against
the float64 reference, the stored value is off by at most E plus half a bf16 step at the fp32 value, so

    |s - ref| <= half_step(|ref| + E) + E

and nothing else is allowed: half_step is the exact half distance between neighbouring bf16 numbers at that magnitude
(2^(floor(log2 x) - 8)), not a relative figure.  E has two parts:
  * the documented error of gelu_pair (csrc/common.h): |erf error| <= 1.5e-7, which enters gelu(gate) = gate * cdf times |gate|
    and a * gelu'(gate) times |a| (cdf and gelu' carry half of it; the bound keeps the documented 1.5e-7);
  * the fp32 arithmetic between the approximation and the rounding: at most six fp32 operations (two fmas and a product
    behind the polynomial, the product with a) and the 1-ulp rcp / exp2, 8 unit round-offs of fp32 = 2^-21 of the value."""
import torch

import gemm_edge_util as U

# (M, ip, K) that reach each form (tests/golden/gemm_dispatch.json lists them; asserted in tests/test_geglu_saved_cpu.py): forward
# the 256 x 256 persistent kernel twice, the 256 x 128 one and the unfused pair twice; backward the persistent, the 256-row and the
# 128 x 128 kernel twice.  No M is a multiple of 256.
FWD = [(4100, 384, 512), (2100, 1408, 512), (2304, 448, 320), (4100, 384, 128), (500, 384, 128)]
BWD = [(41100, 384, 512), (41100, 384, 128), (2304, 640, 320), (500, 384, 128)]

GELU_PAIR_ABS = 1.5e-7          # csrc/common.h, gelu_pair: |error| of its erf
FP32_EVAL_REL = 2.0 ** -21      # 8 x 2^-24


def half_step_bf16(x):
    """half the distance between the two bf16 numbers around |x| (float64 tensor; 0 for x = 0: the bound is then E alone)"""
    x = x.abs()
    e = torch.floor(torch.log2(torch.where(x > 0, x, torch.ones_like(x))))
    return torch.where(x > 0, torch.exp2(e - 8.0), torch.zeros_like(x))


def factors64(h, ip):
    """the saved factors of h = [a | gate] in float64: [gelu(gate) | a * gelu'(gate)]"""
    a, gate = h[:, :ip].double(), h[:, ip:2 * ip].double()
    return torch.cat([U.gelu64(gate), a * U.dgelu64(gate)], 1)


def saved_ref(h, ip):
    """(reference s, bound) from the CHECKED h of the unsaved form"""
    a, gate = h[:, :ip].double(), h[:, ip:2 * ip].double()
    ref = factors64(h, ip)
    E = GELU_PAIR_ABS * torch.cat([gate.abs(), a.abs()], 1) + FP32_EVAL_REL * ref.abs()
    return ref, half_step_bf16(ref.abs() + E) + E


def bwd_vs_unsaved_tol(dh_unsaved, dg, h, ip):
    """|dh_saved - dh_unsaved| <= 2^-7 |dh_unsaved| + the absolute floor of the unsaved form's own bound
    (gemm_edge_util.geglu_bwd_ref: 1e-6 |dg gate| on dh_a, 1e-6 |dg a| on dh_gate)"""
    a, gate = h[:, :ip].double(), h[:, ip:2 * ip].double()
    floor = U.GELU_ABS * torch.cat([(dg * gate).abs(), (dg * a).abs()], 1)
    return 2.0 ** -7 * dh_unsaved.double().abs() + floor
