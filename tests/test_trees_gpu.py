"""The fused forest-walk kernel (K26, ops.trees) against a plain fp64 walk of the attribute lists, one row and
one tree at a time. Inputs come from _ensemble(): random binary trees of a node budget and shape with every
branch mode and both missing-value bits; X is drawn from the grid the thresholds come from, with 10 % NaN, so
<= / < / == / != differ on real rows.

Bounds, u32 = 2^-24, A = sum of |w| over the leaf entries the reference reaches for a score (over T for AVERAGE):
  integer weights   every partial sum is exact in fp32 in any order: scores bit-equal, labels equal
  float weights     |s - ref| <= E_s = (T + 2) u32 A: (T - 1) u32 A for a T-term fp32 sum in any order (Higham,
                    eq. 4.4), one rounding for the division, two for the base add (|base| <= A is asserted)
  post-transforms   |p - ref| <= E_s + 2 e_t + u32: sigmoid and softmax are 1-Lipschitz in the max norm, e_t is
                    the error of torch's fp32 transform against fp64 on the reference scores; labels equal the
                    argmax of the returned probabilities, and the reference label wherever the reference's
                    top-two gap exceeds 2 E_s (at most 1 % of the rows may fall inside)."""
import gc

import numpy as np
import pytest
import torch

from synapseml_amd.onnx import InferenceSession, proto as P, tree_ensemble as TE
from synapseml_amd.onnx.writer import GraphBuilder
from synapseml_amd.ops import trees as TR

U32 = 2.0 ** -24
GRID = np.array([-1.5, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32)
BRANCH = {"BRANCH_LEQ": np.less_equal, "BRANCH_LT": np.less, "BRANCH_GTE": np.greater_equal,
          "BRANCH_GT": np.greater, "BRANCH_EQ": np.equal, "BRANCH_NEQ": np.not_equal}
LAUNCHES = pytest.mark.parametrize("launch", ["rows", "trees"])


def _ensemble(seed, T, F, K, budget=15, *, classifier=True, entries=1, ints=True, kinds=(), labels=None, **extra):
    """attribute lists of T random binary trees of at most ``budget`` nodes (``kinds`` names the first trees:
    "root" only, a "stump", a one-sided "chain" of depth 40); a leaf has 1 .. ``entries`` (id, weight) entries;
    every other tree lists its nodes in reverse, the root last"""
    rng = np.random.default_rng(seed)
    pfx = "class_" if classifier else "target_"
    at = {k: [] for k in ("nodes_treeids", "nodes_nodeids", "nodes_featureids", "nodes_values", "nodes_modes",
                          "nodes_truenodeids", "nodes_falsenodeids", "nodes_missing_value_tracks_true",
                          pfx + "treeids", pfx + "nodeids", pfx + "ids", pfx + "weights")}
    for t in range(T):
        kind = kinds[t] if t < len(kinds) else "random"
        true, false, last = [-1], [-1], 0
        for _ in range({"root": 0, "stump": 1, "chain": 40}.get(kind, (budget - 1) // 2)):
            leaves = [i for i, c in enumerate(true) if c < 0]
            i = last if kind == "chain" else leaves[rng.integers(len(leaves))]
            true[i], false[i], last = len(true), len(true) + 1, len(true)
            true += [-1, -1]
            false += [-1, -1]
        for i in range(len(true))[::-1 if t % 2 else 1]:
            leaf = true[i] < 0
            at["nodes_treeids"].append(t)
            at["nodes_nodeids"].append(i)
            at["nodes_featureids"].append(0 if leaf else int(rng.integers(F)))
            at["nodes_values"].append(0.0 if leaf else float(rng.choice(GRID)))
            at["nodes_modes"].append("LEAF" if leaf else list(BRANCH)[rng.integers(6)])
            at["nodes_truenodeids"].append(max(true[i], 0))
            at["nodes_falsenodeids"].append(max(false[i], 0))
            at["nodes_missing_value_tracks_true"].append(int(rng.integers(2)))
            for e in range(int(rng.integers(1, entries + 1)) if leaf else 0):
                at[pfx + "treeids"].append(t)
                at[pfx + "nodeids"].append(i)
                at[pfx + "ids"].append(K - 1 if not at[pfx + "ids"] else int(rng.integers(K)))
                at[pfx + "weights"].append(float(rng.integers(-4, 5)) if ints else float(np.float32(rng.normal())))
    if classifier:
        at["classlabels_int64s"] = labels or [10 * k + 3 for k in range(max(K, 2))]
    else:
        at["n_targets"] = K
    return {**at, **extra}


def _x(seed, n, F):
    rng = np.random.default_rng(seed)
    X = rng.choice(GRID, (n, F))
    X[rng.random((n, F)) < 0.1] = np.nan
    return X


def _ref(at, X):
    """fp64 (scores after aggregate and base values [n, K], A [n, K]) by walking every tree for every row"""
    pfx = "class_" if "class_ids" in at else "target_"
    at_node = {(t, i): j for j, (t, i) in enumerate(zip(at["nodes_treeids"], at["nodes_nodeids"]))}
    payload = {}
    for t, i, k, w in zip(*(at[pfx + s] for s in ("treeids", "nodeids", "ids", "weights"))):
        payload.setdefault((t, i), []).append((k, float(np.float32(w))))
    T, K = max(at["nodes_treeids"]) + 1, max(at[pfx + "ids"]) + 1
    S, A = np.zeros((len(X), K)), np.zeros((len(X), K))
    for r, x in enumerate(np.asarray(X, np.float64)):
        for t in range(T):
            i, j = 0, at_node[(t, 0)]
            while at["nodes_modes"][j] != "LEAF":
                v, thr = x[at["nodes_featureids"][j]], float(np.float32(at["nodes_values"][j]))
                go = at["nodes_missing_value_tracks_true"][j] if np.isnan(v) else BRANCH[at["nodes_modes"][j]](v, thr)
                i = at["nodes_truenodeids"][j] if go else at["nodes_falsenodeids"][j]
                j = at_node[(t, i)]
            for k, w in payload.get((t, i), []):
                S[r, k] += w
                A[r, k] += abs(w)
    if at.get("aggregate_function") == "AVERAGE":
        S, A = S / T, A / T
    base = np.asarray(at.get("base_values", np.zeros(K)), np.float32).astype(np.float64)
    assert (np.abs(base) <= A).all()
    return S + base, A


def _run(at, X, launch, classifier=True):
    forest = TR.pack(at, classifier)
    out, label = TR.tree_ensemble(X, forest, launch)
    return out.cpu().numpy().astype(np.float64), None if label is None else label.cpu().numpy()


# one row tile + 1 is 257 rows (row-parallel) and 4 rows-per-wave + 1 (tree-parallel; 1030 rows x 2 slices run two
# rows per wave); F = 95 / 191 are the widest rows of the 128- / 64-row tiles, F = 192 is read from global memory;
# 17 trees of 63 nodes are one more than a 1024-node LDS chunk, a 1025-node tree is walked in global memory;
# K = 9 is one more than the register accumulators hold
EXACT = {
    "one": dict(n=1, F=1, T=1, K=1),
    "odd": dict(n=63, F=3, T=7, K=3, entries=3),
    "shapes": dict(n=65, F=28, T=65, K=1, kinds=("root", "stump", "chain", "random", "chain")),
    "tile+1_slab_xglobal": dict(n=257, F=192, T=7, K=9, entries=3),
    "tile128": dict(n=130, F=95, T=3, K=3),
    "tile64": dict(n=65, F=191, T=3, K=9),
    "chunk+1": dict(n=65, F=28, T=17, K=1, budget=63),
    "big_tree": dict(n=5, F=3, T=2, K=3, budget=1025, entries=2),
    "rows_per_wave": dict(n=1030, F=3, T=65, K=1, budget=7),
    "regressor": dict(n=63, F=28, T=7, K=3, classifier=False),
}


@LAUNCHES
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(EXACT))
def test_exact_decisions(case, launch):
    c = dict(EXACT[case])
    n, classifier = c.pop("n"), c.get("classifier", True)
    at = _ensemble(1, **c)
    if case == "shapes":
        assert {*at["nodes_modes"]} == {*BRANCH, "LEAF"} and {*at["nodes_missing_value_tracks_true"]} == {0, 1}
    X = _x(2, n, c["F"])
    S, _ = _ref(at, X)
    out, label = _run(at, torch.from_numpy(X).float().cuda(), launch, classifier)
    if classifier and c["K"] == 1:
        want, idx = np.concatenate([-S, S], 1), (S[:, 0] > 0).astype(int)
    else:
        want, idx = S, np.argmax(S, 1)
    assert out.shape == want.shape and (out == want).all()
    if classifier:
        assert (label == np.asarray(at["classlabels_int64s"])[idx]).all()


@LAUNCHES
@pytest.mark.gpu
@pytest.mark.parametrize("offset", [4, 1], ids=["aligned", "unaligned"])
def test_column_slice(offset, launch):
    """X as a view of a wider tensor: row stride 40 for 28 columns, with and without 16-byte alignment"""
    at = _ensemble(3, T=7, F=28, K=3)
    X = _x(4, 65, 40)
    view = torch.from_numpy(X).float().cuda()[:, offset:offset + 28]
    assert view.stride(0) == 40 and not view.is_contiguous()
    out, label = _run(at, view, launch)
    S, _ = _ref(at, X[:, offset:offset + 28])
    assert (out == S).all() and (label == np.asarray(at["classlabels_int64s"])[np.argmax(S, 1)]).all()


@LAUNCHES
@pytest.mark.gpu
@pytest.mark.parametrize("agg", ["SUM", "AVERAGE"])
@pytest.mark.parametrize("K", [1, 3, 9])
def test_float_weights(K, agg, launch):
    """K = 9 runs without base values: a score no tree adds to has A = 0 and must come out as exactly 0"""
    T = 65
    extra = {"base_values": [0.01 * (-1) ** k for k in range(K)]} if K < 9 else {}
    at = _ensemble(5, T, 28, K, classifier=False, ints=False, aggregate_function=agg, **extra)
    X = _x(6, 65, 28)
    S, A = _ref(at, X)
    out, _ = _run(at, torch.from_numpy(X).float().cuda(), launch, classifier=False)
    err, bound = np.abs(out - S), (T + 2) * U32 * A
    print(f"worst |s - ref| / ((T + 2) u32 A) = {float((err[bound > 0] / bound[bound > 0]).max()):.3f}")
    assert (err <= bound).all()


def _post_ref(S, post, binary):
    """fp64 probabilities of reference scores S, and e_t of torch's fp32 transform on them"""
    cols = np.concatenate([-S, S], 1) if binary else S
    if post == "LOGISTIC":
        p = 1 / (1 + np.exp(-S))
        e_t = np.abs(torch.sigmoid(torch.from_numpy(S).float()).double().numpy() - p).max()
        return (np.concatenate([1 - p, p], 1) if binary else p), cols, e_t
    p = np.exp(S - S.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    return p, cols, np.abs(torch.softmax(torch.from_numpy(S).float(), 1).double().numpy() - p).max()


@LAUNCHES
@pytest.mark.gpu
@pytest.mark.parametrize("post,K", [("LOGISTIC", 1), ("LOGISTIC", 3), ("SOFTMAX", 3)])
def test_post_transforms(post, K, launch):
    T = 7
    labels = [7, 4] if K == 1 else None
    at = _ensemble(7, T, 28, K, ints=False, post_transform=post, labels=labels)
    X = _x(8, 257, 28)
    S, A = _ref(at, X)
    E = ((T + 2) * U32 * A).max(1)
    ref, cols, e_t = _post_ref(S, post, K == 1)
    out, label = _run(at, torch.from_numpy(X).float().cuda(), launch)
    over = float((np.abs(out - ref) - E[:, None]).max())
    print(f"error beyond E_s {over:.3e}, allowed 2 e_t + u32 = {2 * e_t + U32:.3e}")
    assert over <= 2 * e_t + U32
    names = np.asarray(at["classlabels_int64s"])
    assert (label == names[np.argmax(out, 1)]).all()
    top = np.sort(cols, 1)
    clear = top[:, -1] - top[:, -2] > 2 * E
    assert (~clear).mean() <= 0.01
    assert (label[clear] == names[np.argmax(cols, 1)][clear]).all()


def _session_run(op_type, at, X, n_out, device="cuda", use_graph=False, runs=1):
    b = GraphBuilder("trees")
    b.input("X", P.FLOAT32, [None, X.shape[1]])
    outs = b.add(op_type, ["X"], at, n_out=n_out, domain="ai.onnx.ml", out="y")
    for o, ty in zip([outs] if n_out == 1 else outs, [P.INT64, P.FLOAT32] if n_out == 2 else [P.FLOAT32]):
        b.output(o, ty, None)
    sess = InferenceSession(b.to_bytes({"": 13, "ai.onnx.ml": 1}), device=device, use_graph=use_graph)
    res = [[np.asarray(o) for o in sess.run(None, {"X": X})] for _ in range(runs)]
    del sess  # a captured graph and its memory pool go here, with the device idle, not at a later collection
    gc.collect()
    torch.cuda.synchronize()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("op_type", ["TreeEnsembleClassifier", "TreeEnsembleRegressor"])
def test_operator(monkeypatch, op_type):
    classifier = op_type.endswith("Classifier")
    T, K, post = 7, 3, "SOFTMAX" if classifier else "NONE"
    at = _ensemble(9, T, 28, K, classifier=classifier, ints=False, post_transform=post)
    X = _x(10, 65, 28).astype(np.float32)
    S, A = _ref(at, X)
    E = ((T + 2) * U32 * A).max(1)[:, None]
    ref, _, e_t = _post_ref(S, post, False) if classifier else (S, None, 0.0)
    n_out = 2 if classifier else 1
    monkeypatch.setenv("SML_TREES", "0")
    parent = _session_run(op_type, at, X, n_out)[0]
    monkeypatch.setenv("SML_TREES", "1")
    with monkeypatch.context() as mp:
        mp.setattr(TE, "_walk_torch", lambda *a, **k: pytest.fail("fell back to _walk_torch()"))
        eager = _session_run(op_type, at, X, n_out)[0]
        replays = _session_run(op_type, at, X, n_out, use_graph=True, runs=3)
    for got in (eager[-1], parent[-1]):
        assert (np.abs(got.astype(np.float64) - ref) <= E + 2 * e_t + U32).all()
    if classifier:
        assert (eager[0] == np.asarray(at["classlabels_int64s"])[np.argmax(eager[1], 1)]).all()
    for replay in replays:
        for got, want in zip(replay, eager):
            np.testing.assert_array_equal(got, want)
    # a PROBIT node and a host session keep the torch body and return what it returns
    monkeypatch.setattr(TR, "tree_ensemble", lambda *a, **k: pytest.fail("took the kernel"))
    probit = _session_run(op_type, {**at, "post_transform": "PROBIT"}, X, n_out)[0]
    monkeypatch.setenv("SML_TREES", "0")
    for got, want in zip(probit, _session_run(op_type, {**at, "post_transform": "PROBIT"}, X, n_out)[0]):
        np.testing.assert_array_equal(got, want)
    for got, want in zip(_session_run(op_type, at, X, n_out, device="cpu")[0], parent):
        np.testing.assert_allclose(got, want, rtol=0, atol=float((2 * E).max() + 4 * e_t + 2 * U32))


def test_feature_id_out_of_range():
    at = _ensemble(11, T=3, F=5, K=1)
    assert max(at["nodes_featureids"]) == 4
    with pytest.raises(ValueError, match="feature id"):
        TR.tree_ensemble(torch.zeros(2, 4), TR.pack(at, True))
