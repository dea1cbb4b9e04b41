"""Top-k retrieval on the GPU: mca_cosine_topk_f32 through its raw entry point at every listed case (tests/topk_cases.py), compared
exactly with the reference of its semantics (tests/topk_edge_util.py) inside frames; planted galleries; real-valued rows against a
stable sort of the probe layer's matrix (the same fmaf chain, so bit for bit); the rank <-> top-k identity against
mca_cosine_rank_f32; determinism; refusals; metrics.cosine_topk; and retrieve_accel_gpu.py end to end."""
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import topk_cases as TC
import topk_edge_util as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
F32, F64, I32 = torch.float32, torch.float64, torch.int32
BADARG, UNSUPPORTED = -1, -3
DEV = "cuda"
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


@pytest.fixture(scope="module")
def M():
    return importlib.import_module("mca-paper_amd.metrics")


def p(t):
    return None if t is None else t.data_ptr()


def args(H, c, T, O, **over):
    a = dict(q=p(T["q"]), ldq=T["q"].stride(0), qidx=p(T["qidx"]), nq=c["nq"], t=p(T["t"]), ldt=T["t"].stride(0), nt=c["nt"], d=c["d"],
             tvalid=p(T["tvalid"]), exclude=p(T["exclude"]), k=c["k"], ws=O["ws"].data_ptr(), ws_bytes=O["need"], score=O["score"].data_ptr(),
             lds=O["score"].ld, index=O["index"].data_ptr(), ldi=O["index"].ld, stream=H.stream_ptr())
    a.update(over)
    return tuple(a.values())


def launch(H, c, T, O):
    H.call("mca_cosine_topk_f32", *args(H, c, T, O))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ every listed case
@pytest.mark.parametrize("case", TC.TOPK, ids=[c["name"] for c in TC.TOPK])
def test_topk_edges(H, case):
    T, O = U.topk_setup(case, DEV)
    assert H.lib().mca_cosine_topk_workspace(case["nq"], case["nt"], case["k"]) == O["need"]
    launch(H, case, T, O)
    assert int(U.scores64(case, T).abs().max()) < 2 ** 24
    U.topk_check(case, T, O)


# ------------------------------------------------------------------------------------------------ planted galleries
def planted(nq, nt, k, tcol, **opt):
    """d = 1 and every query 1: the score of target j is tcol[j] for every query"""
    c = dict(name=opt.pop("name"), nq=nq, nt=nt, d=1, k=k, qidx=0, tvalid=0, exclude=0)
    c.update(opt)
    T = U.operands(c, torch.ones(nq, 1, device=DEV), tcol.to(DEV).float().reshape(nt, 1), DEV)
    return c, T, U.outputs(c, DEV)


def test_scores_increasing_with_the_index(H):
    """every target displaces an entry: the last k targets, the last first"""
    nt, k = 2 * TC.CHUNK + 1, 10
    c, T, O = planted(65, nt, k, torch.arange(nt), name="planted-increasing")
    launch(H, c, T, O)
    U.topk_check(c, T, O)
    assert O["index"].t[64].tolist() == list(range(nt - 1, nt - 1 - k, -1))


def test_scores_decreasing_with_the_index(H):
    """nothing after the first k enters"""
    nt, k = 2 * TC.CHUNK + 1, 10
    c, T, O = planted(65, nt, k, -torch.arange(nt), name="planted-decreasing")
    launch(H, c, T, O)
    U.topk_check(c, T, O)
    assert O["index"].t[0].tolist() == list(range(k))


@pytest.mark.parametrize("nt,k", [(TC.CHUNK + 1, 10), (70, 64), (5, 64)])
def test_all_scores_equal(H, nt, k):
    c, T, O = planted(3, nt, k, torch.full((nt,), 2.0), name=f"planted-equal-t{nt}k{k}")
    launch(H, c, T, O)
    U.topk_check(c, T, O)
    want = list(range(min(k, nt))) + [-1] * (k - min(k, nt))
    assert all(row == want for row in O["index"].t.tolist())


def test_all_scores_equal_with_a_mask_and_an_exclusion(H):
    nt, k = TC.CHUNK + 1, 10
    c, T, O = planted(6, nt, k, torch.full((nt,), -1.0), name="planted-equal-masked", tvalid=1, exclude=1)
    launch(H, c, T, O)
    U.topk_check(c, T, O)
    # valid: j % 3 != 1; query r excludes target r (query 4 nothing): the first ten of 0 2 3 5 6 8 9 11 12 14 15 without r
    base = [j for j in range(20) if j % 3 != 1]
    for r in range(6):
        assert O["index"].t[r].tolist() == [j for j in base if r == 4 or j != r][:k], r


def test_equal_scores_on_both_sides_of_a_chunk_boundary(H):
    """the best score sits at the end of chunk 0 and, equal, at the start of chunk 1: the merge takes the lower index first"""
    nt, k = 2 * TC.CHUNK, 4
    col = torch.zeros(nt)
    col[[TC.CHUNK - 2, TC.CHUNK - 1, TC.CHUNK, TC.CHUNK + 1, nt - 1]] = 3.0
    c, T, O = planted(2, nt, k, col, name="planted-boundary")
    launch(H, c, T, O)
    U.topk_check(c, T, O)
    assert O["index"].t[1].tolist() == [TC.CHUNK - 2, TC.CHUNK - 1, TC.CHUNK, TC.CHUNK + 1]


def test_a_nan_row_in_the_gallery_is_never_returned(H):
    nt, k, d = 70, 64, 5
    g = U.gen(49, DEV)
    t, q = U.ints((nt, d), g, 2), U.ints((3, d), g, 2)
    t[0] = float("nan")
    t[66, 2] = float("nan")
    c = dict(name="planted-nan", nq=3, nt=nt, d=d, k=k, qidx=0, tvalid=0, exclude=0)
    T, O = U.operands(c, q, t, DEV), U.outputs(c, DEV)
    launch(H, c, T, O)
    U.topk_check(c, T, O)
    got = O["index"].t
    assert not bool(((got == 0) | (got == 66)).any()) and bool((got >= 0).all())          # 68 candidates for 64 places


# ------------------------------------------------------------------------------------------------ real-valued rows
@pytest.fixture(scope="module")
def real(H):
    """normalised randn rows (d = 96, nq = 65, nt = 1025), the full matrix by mca_probe_nt_f32 (act 0, no bias: the same chain),
    the kernel's result for k = 10, and the rank kernel's raw outputs on the same operands; computed once"""
    c = dict(name="real-q65t1025d96k10", nq=65, nt=1025, d=96, k=10, qidx=0, tvalid=0, exclude=0)
    g = U.gen(50, DEV)
    q, t = F.normalize(torch.randn(65, 96, generator=g, device=DEV)), F.normalize(torch.randn(1025, 96, generator=g, device=DEV))
    T, O = U.operands(c, q, t, DEV), U.outputs(c, DEV)
    S = torch.empty(65, 1025, device=DEV)
    H.call("mca_probe_nt_f32", p(T["q"]), T["q"].stride(0), None, p(T["t"]), T["t"].stride(0), None, S.data_ptr(), 1025, 65, 1025, 96, 0, 0.0, 0, 0,
           H.stream_ptr())
    launch(H, c, T, O)
    s_true, rank = torch.empty(65, device=DEV), torch.empty(65, dtype=I32, device=DEV)
    H.call("mca_cosine_rank_f32", p(T["q"]), T["q"].stride(0), None, 65, p(T["t"]), T["t"].stride(0), 1025, 96, s_true.data_ptr(), rank.data_ptr(),
           H.stream_ptr())
    torch.cuda.synchronize()
    return dict(c=c, T=T, O=O, S=S, s_true=s_true, rank=rank)


def test_real_rows_equal_a_stable_sort_of_the_probe_matrix(real):
    c, O, S = real["c"], real["O"], real["S"]
    score, index = U.topk_ref(S, c["k"])                      # fp32 in, fp32 out: the matrix's own bits
    assert torch.equal(O["index"].t, index.to(I32))
    assert torch.equal(O["score"].t.view(I32), score.view(I32)), "score is not the probe layer's value bit for bit"
    order = torch.sort(S, dim=1, descending=True, stable=True)
    assert torch.equal(index, order.indices[:, :c["k"]]) and torch.equal(score.view(I32), order.values[:, :c["k"]].contiguous().view(I32))
    U.topk_check(c, real["T"], O, S=S.double())


def identity(rank, s_true, score, kmax):
    for m in range(1, kmax + 1):
        a, b = rank < m, s_true >= score[:, m - 1]
        assert torch.equal(a, b), f"m = {m}: rank < m and s_true >= score[m - 1] differ at queries {(a != b).nonzero().flatten().tolist()[:8]}"


def test_rank_topk_identity_real(real, M):
    c, O = real["c"], real["O"]
    assert bool((real["s_true"] == real["S"][torch.arange(65), torch.arange(65)]).all())
    identity(real["rank"], real["s_true"], O["score"].t, c["k"])
    srt = torch.sort(real["S"], dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "an exact tie in the real-valued matrix: choose another seed"
    for m in (1, 5, 10):
        assert torch.equal(M.hits_at(O["index"].t.long(), torch.arange(65, device=DEV), m), real["rank"] < m)


@pytest.mark.parametrize("nq,nt,d,k", [(65, 1025, 17, 64), (64, 65, 16, 10), (3, 5, 1, 64)])
def test_rank_topk_identity_integers(H, nq, nt, d, k):
    c = dict(name=f"identity-q{nq}t{nt}d{d}k{k}", nq=nq, nt=nt, d=d, k=k, qidx=0, tvalid=0, exclude=0)
    T, O = U.topk_setup(c, DEV, seed=51)
    launch(H, c, T, O)
    s_true, rank = torch.empty(nq, device=DEV), torch.empty(nq, dtype=I32, device=DEV)
    H.call("mca_cosine_rank_f32", p(T["q"]), T["q"].stride(0), None, nq, p(T["t"]), T["t"].stride(0), nt, d, s_true.data_ptr(), rank.data_ptr(),
           H.stream_ptr())
    torch.cuda.synchronize()
    identity(rank, s_true, O["score"].t, min(k, nt))


# ------------------------------------------------------------------------------------------------ determinism and refusals
def test_two_launches_give_identical_bytes(H):
    c = next(x for x in TC.TOPK if x["nt"] == 2 * TC.CHUNK + 1 and x["k"] == 64)
    T, O1 = U.topk_setup(c, DEV)
    O2 = U.outputs(c, DEV)
    launch(H, c, T, O1)
    launch(H, c, T, O2)
    for key in ("score", "index", "ws"):
        assert torch.equal(O1[key].buf, O2[key].buf), key


def test_refused_calls_store_nothing(H):
    c = dict(name="refused", nq=5, nt=70, d=4, k=10, qidx=0, tvalid=1, exclude=1)
    T, O = U.topk_setup(c, DEV)
    f = H.lib().mca_cosine_topk_f32
    assert f(*args(H, c, T, O, k=0)) == BADARG
    assert f(*args(H, c, T, O, k=65)) == UNSUPPORTED
    assert f(*args(H, c, T, O, d=0)) == BADARG
    assert f(*args(H, c, T, O, ws_bytes=O["need"] - 1)) == BADARG
    assert f(*args(H, c, T, O, ws=None)) == BADARG
    assert f(*args(H, c, T, O, score=None)) == BADARG
    for over in (dict(nq=-1), dict(nt=-1), dict(ldq=3), dict(ldt=3), dict(lds=9), dict(ldi=9), dict(q=None), dict(t=None), dict(index=None)):
        assert f(*args(H, c, T, O, **over)) == BADARG, over
    torch.cuda.synchronize()
    for key in ("score", "index", "ws"):
        U.untouched(O[key], f"refused {key}")
    assert f(*args(H, c, T, O, nq=0)) == 0          # no query: nothing launched
    torch.cuda.synchronize()
    for key in ("score", "index", "ws"):
        U.untouched(O[key], f"nq = 0: {key}")


def test_no_target_fills_every_row_with_padding(H):
    c = dict(name="no-target", nq=5, nt=1, d=4, k=3, qidx=0, tvalid=0, exclude=0)
    T, O = U.topk_setup(c, DEV)
    assert H.lib().mca_cosine_topk_workspace(5, 0, 3) == 0
    assert H.lib().mca_cosine_topk_f32(*args(H, c, T, O, nt=0, ws=None, ws_bytes=0)) == 0
    torch.cuda.synchronize()
    assert bool((O["index"].t == -1).all()) and bool((O["score"].t == NEG_INF).all())
    U.assert_guard_intact(O["score"], "score"), U.assert_guard_intact(O["index"], "index"), U.untouched(O["ws"], "ws")


# ------------------------------------------------------------------------------------------------ the python surface
def test_metrics_cosine_topk_against_the_raw_entry_point(H, M):
    g = torch.Generator().manual_seed(52)
    q, t = torch.randn(70, 24, generator=g), torch.randn(1100, 24, generator=g) * 3.0          # cpu inputs, rows of any norm
    sel = torch.tensor([69, 3, 3, 0, 41])
    mask = torch.arange(1100) % 4 != 2
    ex = torch.tensor([5, -1, 0, 1099, 7])
    c = dict(name="surface", nq=5, nt=1100, d=24, k=7, qidx=1, tvalid=1, exclude=1)
    T = dict(q=M.normalize_rows(q), t=M.normalize_rows(t), qidx=sel.to(DEV, I32), tvalid=mask.to(DEV, torch.uint8), exclude=ex.to(DEV, I32))
    O = U.outputs(c, DEV)
    launch(H, c, T, O)
    score, index = M.cosine_topk(q, t, 7, query_index=sel, target_mask=mask, exclude=ex)
    assert score.dtype == F32 and index.dtype == torch.int64 and score.shape == index.shape == (5, 7) and score.device.type == "cuda"
    assert torch.equal(index, O["index"].t.long()) and torch.equal(score.view(I32), O["score"].t.contiguous().view(I32))
    assert not bool(((index % 4) == 2).any()) and 5 not in index[0].tolist()
    # and plainly: every option None, against a float64 restatement (no tie between neighbours at fp32 resolution)
    score, index = M.cosine_topk(q, t, 7)
    S = F.normalize(q.double()) @ F.normalize(t.double()).T
    want = torch.sort(S, dim=1, descending=True, stable=True)
    assert torch.equal(index.cpu(), want.indices[:, :7]) and float((score.cpu().double() - want.values[:, :7]).abs().max()) < 1e-6
    with pytest.raises(ValueError, match="k must be"):
        M.cosine_topk(q, t, 65)


# ------------------------------------------------------------------------------------------------ the script
def _run(args_, timeout=240):
    return subprocess.run([sys.executable, *args_], cwd=REPO, capture_output=True, text=True, timeout=timeout)


def _brute(qe, te, sel, mask, k):
    """float64 cosine top-k of rows sel of qe against the rows of te the mask admits"""
    S = F.normalize(qe.double())[sel] @ F.normalize(te.double()).T
    S[:, ~mask] = float("nan")
    return U.topk_ref(S, k)


def test_retrieve_script_end_to_end(M, tmp_path):
    g = torch.Generator().manual_seed(53)
    emb = tmp_path / "emb"
    emb.mkdir()
    n, D, names = {"train": 40, "eval": 24}, 16, ("audio", "text", "fusion")
    E, P, Y = {}, {}, {}
    for split in ("train", "eval"):
        base = torch.randn(n[split], D, generator=g)
        E[split] = {m: base + 0.5 * torch.randn(n[split], D, generator=g) for m in names}
        E[split][frozenset(("audio", "text"))] = base.clone()          # a non-string key, as infer_accel_gpu.py writes: ignored
        P[split] = {"audio": torch.arange(n[split]) % 4 != 1, "text": torch.arange(n[split]) % 5 != 2}          # gaps; fusion has no mask
        Y[split] = torch.stack([torch.randn(n[split], generator=g), (base[:, 0] > 0).float(), base[:, 1]], 1)
        torch.save(E[split], emb / f"{split}_embeddings.pt")
        torch.save(P[split], emb / f"{split}_masks.pt")
        torch.save(Y[split], emb / f"{split}_labels.pt")
    pres = lambda split, m: P[split].get(m, torch.ones(n[split], dtype=torch.bool))
    runs = {"bce": "task: 1\nloss_type: BCE\nknn_k: 5\n", "mse": "task: 2\nloss_type: MSE\nretrieval_k: 12\n", "none": "task: -1\n"}
    logs, saved, outs = {}, {}, {}
    for name, body in runs.items():
        out = tmp_path / name
        y = tmp_path / f"{name}.yaml"
        y.write_text(f"embedding_dir: {emb}\noutput_dir: {out}\n" + body)
        r = _run(["retrieve_accel_gpu.py", str(y)])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        logs[name] = {k: v for line in open(out / "log.jsonl") for k, v in json.loads(line).items()}
        saved[name] = torch.load(out / "retrieval.pt", weights_only=False)
        outs[name] = r.stdout
    pairs = [(a, b) for a in names for b in names if a != b]
    retrieval_keys = {f"{s}_{a}_to_{b}_{x}" for s in ("train", "eval") for a, b in pairs for x in ("hit1", "hit5", "hit10", "n")}
    binary = {"precision", "recall", "accuracy", "cm", "f1", "specificity", "auroc", "auprc"}
    assert set(logs["bce"]) == retrieval_keys | {f"knn_{m}_{x}" for m in names for x in binary}
    assert set(logs["mse"]) == retrieval_keys | {f"knn_{m}_pearson" for m in names}
    assert set(logs["none"]) == retrieval_keys and "kNN readout skipped" in outs["none"] and saved["none"]["knn"] == {}
    # retrieval.pt and the hit rates against brute force
    for name, k in (("bce", 10), ("mse", 12)):
        for split in ("train", "eval"):
            assert set(saved[name]["retrieval"][split]) == {f"{a}_to_{b}" for a, b in pairs}
            for a, b in pairs:
                got = saved[name]["retrieval"][split][f"{a}_to_{b}"]
                sel = torch.nonzero(pres(split, a) & pres(split, b)).reshape(-1)
                score, index = _brute(E[split][a], E[split][b], sel, pres(split, b), k)
                assert torch.equal(got["query"], sel) and got["index"].dtype == I32 and got["index"].shape == (sel.numel(), k)
                assert torch.equal(got["index"].long(), index), (name, split, a, b)
                assert float((got["score"].double() - score).abs().max()) < 1e-6
                assert logs[name][f"{split}_{a}_to_{b}_n"] == sel.numel()
                for m in (1, 5, 10):
                    want = (index[:, :m] == sel[:, None]).any(1).float().mean().item()
                    assert abs(logs[name][f"{split}_{a}_to_{b}_hit{m}"] - want) < 1e-6
    # the kNN block: neighbour means by brute force, through the probe's own metric functions
    for name, k, col in (("bce", 5, 1), ("mse", 10, 2)):
        for m in names:
            sel = torch.nonzero(pres("eval", m)).reshape(-1)
            score, index = _brute(E["eval"][m], E["train"][m], sel, pres("train", m), k)
            got = saved[name]["knn"][m]
            assert torch.equal(got["query"], sel) and torch.equal(got["index"].long(), index)
            pred = Y["train"][:, col][index].mean(1)
            assert float((got["pred"] - pred).abs().max()) < 1e-6
            if name == "bce":
                want = M.binary_metrics(pred, Y["eval"][sel, col])
                for x, v in want.items():
                    if x == "cm":
                        assert logs[name][f"knn_{m}_cm"] == v.tolist()
                    else:
                        assert abs(logs[name][f"knn_{m}_{x}"] - v.item()) < 1e-6, (m, x)
            else:
                assert abs(logs[name][f"knn_{m}_pearson"] - M.pearson(pred, Y["eval"][sel, col]).item()) < 1e-5
    # one process only
    env = dict(os.environ, WORLD_SIZE="2")
    r = subprocess.run([sys.executable, "retrieve_accel_gpu.py", str(tmp_path / "none.yaml")], cwd=REPO, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "one process" in r.stderr
