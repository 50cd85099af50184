"""Fused MFMA top-k inner-product search (K23, ops.mips) against a plain numpy fp64 reference, and KNN /
ConditionalKNN served by it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from synapseml_amd import nn  # noqa: E402
from synapseml_amd.core.dataframe import DataFrame  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(Q, K, k, splits=None, key_label=None, allow=None):
    from synapseml_amd.ops import mips

    dev = lambda x: None if x is None else torch.as_tensor(x, device="cuda")  # noqa: E731
    v, i = mips.topk(dev(Q.astype(np.float32)), dev(K.astype(np.float32)), k, dev(key_label), dev(allow), splits=splits)
    return v.cpu().numpy(), i.cpu().numpy()


def _reference(S, k, eligible=None):
    """stable descending top-k of fp64 scores [M, N]; (vals, idx) padded with -inf / -1"""
    if eligible is not None:
        S = np.where(eligible, S, -np.inf)
    order = np.argsort(-S, kind="stable")[:, :k]
    vals = np.take_along_axis(S, order, 1)
    idx = np.where(np.isfinite(vals), order, -1)
    pad = k - idx.shape[1]
    return np.pad(vals, ((0, 0), (0, pad)), constant_values=-np.inf), np.pad(idx, ((0, 0), (0, pad)), constant_values=-1)


def _ints(rng, *shape):
    return rng.integers(-4, 5, size=shape).astype(np.float64)


# k > N (with and without ragged D), N one past a key tile with D % 4 != 0, D = 1 (ties everywhere, across the
# split boundaries), every split holding one tile, splits clamped to the tile count
@pytest.mark.parametrize("M,N,D,k,splits", [
    (1, 1, 1, 1, 1), (1, 1, 3, 5, 1), (63, 127, 3, 5, 1), (65, 129, 33, 64, 1), (63, 300, 1, 64, 3),
    (65, 300, 100, 5, 3), (1, 129, 100, 64, 3), (65, 127, 33, 64, 3)])
def test_exact_integer_data(M, N, D, k, splits):
    rng = np.random.default_rng(M * 1000 + N + D)
    Q, K = _ints(rng, M, D), _ints(rng, N, D)
    vals, idx = _run(Q, K, k, splits)
    rv, ri = _reference(Q @ K.T, k)
    assert np.array_equal(idx, ri)
    assert np.array_equal(vals.astype(np.float64), rv)


@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("descending", [False, True])
def test_adversarial_key_order(k, descending):
    """keys c_n * e with c_n monotone in n: for half the queries every key beats every threshold"""
    rng = np.random.default_rng(7)
    N, M = 400, 65
    c = np.arange(N, dtype=np.float64) - 200
    K = np.outer(c[::-1] if descending else c, np.array([1.0, 2.0, 0.0, 1.0]))
    Q = _ints(rng, M, 4)
    vals, idx = _run(Q, K, k, 1)
    rv, ri = _reference(Q @ K.T, k)
    assert np.array_equal(idx, ri)
    assert np.array_equal(vals.astype(np.float64), rv)


@pytest.mark.parametrize("labels,N,splits", [(1, 3, 1), (5, 300, 1), (70, 300, 1), (70, 300, 3)])
def test_conditioner(labels, N, splits):
    rng = np.random.default_rng(labels)
    M, D, k = 65, 8, 5
    Q, K = _ints(rng, M, D), _ints(rng, N, D)
    key_label = rng.integers(0, max(labels - 1, 1), size=N).astype(np.int32)
    key_label[:2] = labels - 1  # the last label sits on two keys only: fewer than k eligible
    allowed = rng.random((M, labels)) < 0.3
    allowed[0] = False
    allowed[1] = np.arange(labels) == 0
    allowed[2] = True
    allowed[3] = np.arange(labels) == labels - 1
    words = (labels + 31) // 32
    bits = np.zeros((M, words * 32), bool)
    bits[:, :labels] = allowed
    allow = np.packbits(bits, axis=1, bitorder="little").view(np.uint32).view(np.int32)
    vals, idx = _run(Q, K, k, splits, key_label, allow)
    rv, ri = _reference(Q @ K.T, k, allowed[:, key_label])
    assert np.array_equal(idx, ri)
    assert np.array_equal(vals.astype(np.float64), rv)
    assert (idx[0] == -1).all() and np.isneginf(vals[0]).all() and (idx[3] >= 0).sum() == min(k, (key_label == labels - 1).sum())


@pytest.mark.parametrize("M,N,D,k,splits", [(65, 300, 100, 5, 1), (63, 129, 33, 64, 2), (1, 127, 3, 5, 1)])
def test_gaussian_value_bound(M, N, D, k, splits):
    """Every slot within e = D 2^-23 sum_i |q_i k_i| of the fp64 reference, by rank and by index: at most D
    fp32 roundings (relative 2^-24) of the running sum, doubled for the undocumented order inside the MFMA.
    Worst observed ratio to e on an MI355X: 0.104 by rank, 0.121 by index (the D = 3 case)."""
    rng = np.random.default_rng(D)
    Q = rng.normal(size=(M, D)).astype(np.float32).astype(np.float64)
    K = rng.normal(size=(N, D)).astype(np.float32).astype(np.float64)
    vals, idx = _run(Q, K, k, splits)
    S, E = Q @ K.T, D * 2.0 ** -23 * (np.abs(Q) @ np.abs(K).T)
    assert (idx >= 0).all()
    by_rank = np.abs(vals - _reference(S, k)[0]) / E.max(1, keepdims=True)
    by_index = np.abs(vals - np.take_along_axis(S, idx, 1)) / np.take_along_axis(E, idx, 1)
    print(f"mips worst ratio to e: by rank {by_rank.max():.3g}, by index {by_index.max():.3g}")
    assert by_rank.max() <= 1 and by_index.max() <= 1


@pytest.mark.parametrize("fused", [True, False])
def test_knn_stages(fused, monkeypatch):
    rng = np.random.default_rng(11)
    K, Qm = _ints(rng, 300, 6), _ints(rng, 70, 6)
    if not fused:  # torch.topk promises no tie order: column 0 makes every score of a query distinct
        K[:, 1:] *= 1000
        K[:, 0], Qm[:, 0] = rng.permutation(300), rng.choice([-1.0, 1.0], 70)
    lab = [f"l{i % 7}" for i in range(300)]
    df = DataFrame({"features": K, "values": np.arange(300), "label": np.array(lab, dtype=object)})
    cond = np.empty(70, dtype=object)
    for i in range(70):
        cond[i] = [["l1"], ["l0", "l5", "absent"], [], lab[:7]][i % 4]
    qdf = DataFrame({"features": Qm, "conditioner": cond})
    if fused:
        def torch_path(*a, **kw):
            raise AssertionError("the torch path served the call")
        monkeypatch.setattr(nn, "_device_mips", torch_path)
    else:
        monkeypatch.setenv("SML_MIPS", "0")
    m, cm = nn.KNN(k=3).fit(df), nn.ConditionalKNN(k=4).fit(df)
    got, cgot = m.transform(qdf)[m.getOutputCol()], cm.transform(qdf)[cm.getOutputCol()]
    bt, cbt = m.getBallTree(), cm.getBallTree()
    for r in range(70):
        want = [{"value": bt.values[b.index], "distance": b.distance} for b in bt.findMaximumInnerProducts(Qm[r], 3)]
        assert got[r] == want
        cwant = [{"value": cbt.values[b.index], "distance": b.distance, "label": cbt.labels[b.index]}
                 for b in cbt.findMaximumInnerProducts(Qm[r], set(cond[r]), 4)]
        assert cgot[r] == cwant
