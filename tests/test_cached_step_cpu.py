"""The gradient-cached step's pure parts (mca-paper_amd/cached.py), without a GPU: the chunk plan, the order of the launches, the
YAML key and the script's refusals."""
import importlib

import pytest

cached = importlib.import_module("mca-paper_amd.cached")


def test_chunk_plan():
    assert cached.chunk_plan(6, 2) == [(0, 2), (2, 4), (4, 6)] and cached.chunk_plan(6, 3) == [(0, 3), (3, 6)] and cached.chunk_plan(5, 5) == [(0, 5)]
    for B, mb in ((7, 2), (0, 2), (2, 4), (4, 0), (4, -2)):
        with pytest.raises(ValueError, match="micro_batch"):
            cached.chunk_plan(B, mb)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_pass_plan_runs_2n_minus_1_forwards_and_n_backwards(n):
    plan = cached.pass_plan(n)
    fwd, bwd = [i for k, i in plan if k == "forward"], [i for k, i in plan if k == "backward"]
    assert len(fwd) == 2 * n - 1 and len(bwd) == n and [k for k, _ in plan].count("loss") == 1
    at = plan.index(("loss", -1))
    assert plan[:at] == [("forward", i) for i in range(n)]          # pass 1 in order
    assert bwd == list(reversed(range(n)))                          # pass 2 in reverse
    assert plan[at + 1] == ("backward", n - 1)                      # the last chunk's activations are still there
    for i in range(n - 1):                                          # every other chunk: its forward directly before its backward
        assert plan[plan.index(("backward", i)) - 1] == ("forward", i)


def test_yaml_key():
    assert cached.grad_cache_chunks({}) == 1 and cached.grad_cache_chunks({"grad_cache_chunks": 1}) == 1
    assert cached.grad_cache_chunks({"grad_cache_chunks": 4}) == 4 and cached.grad_cache_chunks({"grad_cache_chunks": None}) == 1
    for bad in (0, -1, 2.0, "2", True):
        with pytest.raises(ValueError, match="grad_cache_chunks"):
            cached.grad_cache_chunks({"grad_cache_chunks": bad})
    config = importlib.import_module("mca-paper_amd.config")
    assert "grad_cache_chunks" not in config.default_train_config()          # the defaults keep the reference's keys


def test_script_refusals_name_both_options():
    cached.refuse_with(1, True, 4)
    cached.refuse_with(2, False, 1)
    with pytest.raises(SystemExit, match=r"grad_cache_chunks.*--graph"):
        cached.refuse_with(2, True, 1)
    with pytest.raises(SystemExit, match=r"grad_cache_chunks.*rank"):
        cached.refuse_with(2, False, 2)


def test_grouping_drops_the_leftover():
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    train = importlib.import_module("train_accel_gpu")
    assert list(train.grouped(iter(range(7)), 3)) == [[0, 1, 2], [3, 4, 5]] and list(train.grouped(iter(range(2)), 3)) == []
