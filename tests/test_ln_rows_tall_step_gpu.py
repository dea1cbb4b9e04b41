"""FusionEngine.ln_rows_tall at step level, by the method of tests/test_ln_rows_step_gpu.py (whose helpers are used here): the CMU
configuration at depth 1, b = 2 (T = 5,076 token rows), one forward + backward with the 160-row kernel forced (knob 15 = 2: at this
size the height rule itself picks 128 rows, and the engine then keeps mca_gemm_nt_res_lnbwd) and one with MCA_DEBUG's
ln_rows_tall switched off.  Both runs pin the other atomic orders as that test does (knobs 3 = 1 and 14 = 1, every modality
present, the encoder input norms' parameter gradients through the fixed-order form).  The 160-row kernel produces dx and its bf16
copy bit for bit (tests/test_gemm_rows_tall_gpu.py), so the loss, the pooled outputs and every gradient but the trunk norm gammas
are the same bits; the gammas - added with fp32 atomics, 32 workgroups against 40 - agree to the atomic-order bound."""
import copy
import importlib

import pytest
import torch

from test_ln_rows_step_gpu import B, GAMMA_REL, counting, is_gamma, ordered_param_norms
from util_small import rel_err

pytestmark = pytest.mark.gpu
OLD, TALL = "mca_gemm_nt_res_lnbwd", "mca_gemm_nt_res_lnbwd_tall"


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("mca-paper_amd")


def run(P, cfg, batch, tall, height):
    H = importlib.import_module("mca-paper_amd.hip")
    torch.manual_seed(43)
    model = P.MCA(**copy.deepcopy(cfg)).cuda()
    eng = model.engine
    eng.check_finite = False
    eng.ln_rows_tall = tall
    with H.knobs(**{"k3": 1, "k14": 1, f"k{H.KNOB_ROWS_HEIGHT}": height}), counting(H, OLD) as old, counting(H, TALL) as new, \
            ordered_param_norms(H) as ordered:
        out = model(batch)
        out["loss"].backward()
        torch.cuda.synchronize()
    assert ordered.n > 0
    return dict(out={k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)},
                grads={n: p.grad.detach().clone() for n, p in model.named_parameters()}, old=old.n, new=new.n,
                rule=eng.ln_rows_backward(B * eng.N), T=B * eng.N)


@pytest.fixture(scope="module")
def steps(P):
    cfg = dict(P.config.cmu_model_config(batch_size=B), depth=1)
    batch = P.data.synthetic_batch(cfg, B, seed=1234, lengths="uniform", p_drop=0.0, device="cuda")
    return dict(tall=run(P, cfg, batch, True, 2), off=run(P, cfg, batch, False, 2), rule=run(P, cfg, batch, True, 0))


def test_the_engine_calls_the_tall_entry_point_only_for_the_160_row_plan(steps):
    tall, off, rule = steps["tall"], steps["off"], steps["rule"]
    assert tall["T"] == 5076 and tall["rule"] and off["rule"] and rule["rule"]
    assert (tall["new"], tall["old"]) == (3, 0)          # both norms of the layer and the final norm, 160 rows forced
    assert (off["new"], off["old"]) == (0, 3)            # ln_rows_tall off: the 128-row entry point whatever the knob says
    assert (rule["new"], rule["old"]) == (0, 3)          # the rule at b = 2: 128 rows, so the old name is called


def test_loss_outputs_and_gradients_are_bit_identical(steps):
    for other in ("off", "rule"):
        on, off = steps["tall"], steps[other]
        assert set(on["out"]) == set(off["out"]) and "loss" in on["out"] and len(on["out"]) > 1
        for k, v in off["out"].items():
            assert torch.equal(on["out"][k], v), k
        names = [n for n in off["grads"] if not is_gamma(n)]
        assert len(names) >= 33 and len(off["grads"]) - len(names) <= 4
        differing = {n: rel_err(on["grads"][n], off["grads"][n]) for n in names if not torch.equal(on["grads"][n], off["grads"][n])}
        print(f"ln rows tall step: {len(names)} gradients compared bit for bit against '{other}', {len(differing)} differ: {differing}")
        assert not differing, differing
        assert all(bool(torch.isfinite(g).all()) for g in on["grads"].values()) and float(on["grads"]["layers.0.norm.gamma"].abs().max()) > 0


def test_gammas_agree_to_the_atomic_order_bound(steps):
    on, off = steps["tall"], steps["off"]
    gammas = [n for n in off["grads"] if is_gamma(n)]
    assert {"norm.gamma", "layers.0.norm.gamma"} <= set(gammas), gammas          # the final norm and the layer's shared norm
    worst = {n: rel_err(on["grads"][n], off["grads"][n]) for n in gammas}
    print(f"ln rows tall step: LayerNorm parameter gradients, relative difference 160 rows against 128: {worst}")
    for n, d in worst.items():
        assert d <= GAMMA_REL, (n, d)
