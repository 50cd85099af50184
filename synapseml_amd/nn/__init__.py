"""Maximum-inner-product nearest neighbours (reference: core/.../nn/
{BallTree, ConditionalBallTree, KNN, ConditionalKNN}.scala).

``BallTree`` / ``ConditionalBallTree`` reproduce the reference's exact
branch-and-bound search on the host. ``KNNModel.transform`` is exact MIPS as
a dense scan of all keys on the device when a GPU is visible — on the MI355X
that beats tree traversal — and falls back to the ball tree on the host. The
device scan is the fused MFMA top-k kernel (K23, ``ops.mips``): scores stay in
registers, the conditioner is a label id per key and a bitset per query, and
the fp32 keys are uploaded once per tree. ``k`` > 64, more than
``ops.mips.MAX_LABELS`` labels, unconditional keys wider than 512, non-finite
data or ``SML_MIPS=0`` take the blocked GEMM + ``torch.topk`` path
(``_device_mips``) instead."""
from __future__ import annotations

import heapq
import os
from typing import Any, Dict, List, Optional, Sequence, Set

import numpy as np

from ..core.contracts import HasFeaturesCol, HasLabelCol, HasOutputCol
from ..core.dataframe import DataFrame
from ..core.linalg import as_matrix
from ..core.params import Param, Params, TypeConverters as T
from ..core.pipeline import Estimator, Model


class _Node:
    __slots__ = ("idx", "center", "radius", "left", "right", "labels")

    def __init__(self, idx, center, radius, left=None, right=None):
        self.idx, self.center, self.radius, self.left, self.right = idx, center, radius, left, right
        self.labels = None


class BestMatch:
    __slots__ = ("index", "distance")

    def __init__(self, index: int, distance: float):
        self.index, self.distance = index, distance

    def __repr__(self):
        return f"BestMatch({self.index}, {self.distance:.4g})"


class BallTree:
    """Ball tree for maximum inner product search: bound = q·c + |q|·r."""

    def __init__(self, keys, values: Sequence[Any], leafSize: int = 50):  # noqa: N803
        self.keys = np.asarray(keys, dtype=np.float64)
        self.values = list(values)
        self.leaf_size = leafSize
        self.root = self._build(np.arange(len(self.keys)))

    def __getstate__(self):
        # the device copy of the keys (_device_topk) is rebuilt on demand, never pickled or saved
        return {k: v for k, v in self.__dict__.items() if k != "_dev"}

    def _build(self, idx: np.ndarray) -> _Node:
        pts = self.keys[idx]
        center = pts.mean(0)
        radius = float(np.sqrt(((pts - center) ** 2).sum(1).max())) if len(idx) else 0.0
        if len(idx) <= self.leaf_size:
            return _Node(idx, center, radius)
        # two far-apart pivots
        a = int(np.argmax(((pts - pts[0]) ** 2).sum(1)))
        b = int(np.argmax(((pts - pts[a]) ** 2).sum(1)))
        da = ((pts - pts[a]) ** 2).sum(1)
        db = ((pts - pts[b]) ** 2).sum(1)
        left = idx[da <= db]
        right = idx[da > db]
        if len(left) == 0 or len(right) == 0:
            return _Node(idx, center, radius)
        return _Node(idx, center, radius, self._build(left), self._build(right))

    @staticmethod
    def _bound(q, qn, node):
        return float(q @ node.center) + qn * node.radius

    def _search(self, q, k, node, heap, allowed: Optional[Set[int]] = None):
        qn = float(np.linalg.norm(q))
        if len(heap) == k and heap[0][0] > self._bound(q, qn, node):
            return
        if node.left is None:
            ids = node.idx if allowed is None else [i for i in node.idx if i in allowed]
            for i in ids:
                d = float(q @ self.keys[i])
                item = (d, -int(i))
                if len(heap) < k:
                    heapq.heappush(heap, item)
                elif item > heap[0]:
                    heapq.heapreplace(heap, item)
            return
        children = sorted([node.left, node.right], key=lambda n: -self._bound(q, qn, n))
        for c in children:
            self._search(q, k, c, heap, allowed)

    def findMaximumInnerProducts(self, queryPoint, k: int = 1) -> List[BestMatch]:  # noqa: N802,N803
        heap: list = []
        self._search(np.asarray(queryPoint, np.float64), k, self.root, heap)
        return [BestMatch(-i, d) for d, i in sorted(heap, reverse=True)]


class ConditionalBallTree(BallTree):
    def __init__(self, keys, values, labels: Sequence[Any], leafSize: int = 50):  # noqa: N803
        self.labels = list(labels)
        super().__init__(keys, values, leafSize)

    def save(self, filename: str) -> None:
        """keys, values, labels and leaf size as JSON (rebuilt deterministically on load; reference
        nn/ConditionalBallTree.py save / load)"""
        import json

        with open(filename, "w") as f:
            json.dump({"keys": self.keys.tolist(), "values": list(self.values), "labels": list(self.labels),
                       "leafSize": self.leaf_size}, f)

    @staticmethod
    def load(filename: str) -> "ConditionalBallTree":
        import json

        with open(filename) as f:
            d = json.load(f)
        return ConditionalBallTree(np.asarray(d["keys"], np.float64), d["values"], d["labels"], d["leafSize"])

    def findMaximumInnerProducts(self, queryPoint, conditioner: Set[Any], k: int = 1):  # noqa: N802,N803
        allowed = {i for i, l in enumerate(self.labels) if l in conditioner}
        heap: list = []
        if allowed:
            self._search(np.asarray(queryPoint, np.float64), k, self.root, heap, allowed)
        return [BestMatch(-i, d) for d, i in sorted(heap, reverse=True)]


def _device_mips(Q: np.ndarray, K: np.ndarray, k: int, mask: Optional[np.ndarray] = None, block: int = 8192):
    """Exact top-k inner products via blocked device GEMM; ties broken by smaller index like the tree."""
    import torch

    dev = torch.device("cuda")
    Kt = torch.as_tensor(K, dtype=torch.float32, device=dev)
    out_v, out_i = [], []
    for s in range(0, len(Q), block):
        q = torch.as_tensor(Q[s:s + block], dtype=torch.float32, device=dev)
        sc = q @ Kt.T
        if mask is not None:
            sc = sc.masked_fill(~torch.as_tensor(mask[s:s + block], device=dev), float("-inf"))
        v, i = torch.topk(sc, min(k, K.shape[0]), dim=1)
        out_v.append(v.cpu().numpy())
        out_i.append(i.cpu().numpy())
    return np.concatenate(out_v), np.concatenate(out_i)


# Widest unconditional keys the fused kernel serves: at D = 2048 it was slower than the torch path's device steps
# at every measured shape, at D = 128 faster wherever the queries fill the device (profiles/r9/mips); nothing was
# measured in between. The conditional stage always takes the kernel: its torch path builds a Q x N mask on
# the host, which costs more than either device path.
_MIPS_MAX_D = 512


def _device_keys(bt: "BallTree", conditional: bool):
    """The tree's device-side operands, cached on the tree per device: fp32 keys, whether they are finite and,
    for a conditional tree, the dense label ids (dict label -> id, int32 id per key)"""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    cache = bt.__dict__.setdefault("_dev", {})
    ent = cache.get(dev)
    if ent is None:
        ent = {"keys": torch.as_tensor(bt.keys, dtype=torch.float32, device=dev),
               "finite": bool(np.isfinite(bt.keys).all())}
        cache[dev] = ent
    if conditional and "ids" not in ent:
        ids: Dict[Any, int] = {}
        for l in bt.labels:
            ids.setdefault(l, len(ids))
        ent["ids"] = ids
        ent["key_label"] = torch.as_tensor(np.fromiter((ids[l] for l in bt.labels), np.int32, len(bt.labels)),
                                           device=dev)
    return ent


def _device_topk(bt: "BallTree", Q: np.ndarray, k: int, conds: Optional[List[Set[Any]]] = None, block: int = 8192):
    """Top-k inner products of every query against the tree's keys on the device: (vals, idx) with -inf / -1 in
    the slots that cannot be filled, from the fused kernel (ops.mips); None when the kernel does not take the
    problem (the caller then runs ``_device_mips``)."""
    if os.environ.get("SML_MIPS", "1") == "0" or not 1 <= k <= 64 or not len(bt.keys):
        return None
    if conds is None and bt.keys.shape[1] > _MIPS_MAX_D:
        return None
    import torch

    from ..ops import mips

    ent = _device_keys(bt, conds is not None)
    if not ent["finite"] or not np.isfinite(Q).all():
        return None
    words = 0
    if conds is not None:
        if len(ent["ids"]) > mips.MAX_LABELS:
            return None
        words = mips.allow_words(len(ent["ids"]))
    out_v, out_i = [], []
    for s in range(0, len(Q), block):
        q = torch.as_tensor(Q[s:s + block], dtype=torch.float32, device=ent["keys"].device)
        key_label = allow = None
        if conds is not None:
            bits = np.zeros((len(q), words), np.uint32)
            ids = ent["ids"]
            for r, c in enumerate(conds[s:s + block]):
                for l in c:
                    i = ids.get(l)
                    if i is not None:
                        bits[r, i >> 5] |= np.uint32(1 << (i & 31))
            key_label, allow = ent["key_label"], torch.as_tensor(bits.view(np.int32), device=q.device)
        if not mips.supported(q, ent["keys"], k, key_label, allow):
            return None
        v, i = mips.topk(q, ent["keys"], k, key_label, allow)
        out_v.append(v.cpu().numpy())
        out_i.append(i.cpu().numpy())
    return np.concatenate(out_v), np.concatenate(out_i)


def _use_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # pragma: no cover
        return False


class _KNNParams(HasFeaturesCol, HasOutputCol):
    valuesCol = Param("column holding values for each feature (key) that will be returned when queried",
                      "values", T.toString)
    leafSize = Param("max size of the leaves of the tree", 50, T.toInt)
    k = Param("number of matches to return", 5, T.toInt)


def _obj(values) -> np.ndarray:
    arr = np.empty(len(values), dtype=object)
    for i, v in enumerate(values):
        arr[i] = v
    return arr


class KNNModel(Model, _KNNParams):
    ballTree = Param("the ballTree model used for performing queries", None, complex=True)

    def _transform(self, df):
        bt: BallTree = self.getBallTree()
        Q = as_matrix(df[self.getFeaturesCol()])
        k = self.getK()
        res = []
        if _use_gpu() and len(Q):
            fused = _device_topk(bt, Q, k)
            vals, idx = fused if fused is not None else _device_mips(Q, bt.keys, k)
            for r in range(len(Q)):
                res.append([{"value": bt.values[int(i)], "distance": float(v)} for v, i in zip(vals[r], idx[r])
                            if i >= 0])
        else:
            for q in Q:
                res.append([{"value": bt.values[m.index], "distance": m.distance}
                            for m in bt.findMaximumInnerProducts(q, k)])
        return df.withColumn(self.getOutputCol(), _obj(res))


class KNN(Estimator, _KNNParams):
    def __init__(self, **kw):
        super().__init__(**kw)
        self._setDefault(outputCol=self.uid + "_output")

    def _fit(self, df):
        bt = BallTree(as_matrix(df[self.getFeaturesCol()]), df[self.getValuesCol()].tolist(), self.getLeafSize())
        m = KNNModel(featuresCol=self.getFeaturesCol(), valuesCol=self.getValuesCol(), outputCol=self.getOutputCol(),
                     k=self.getK(), leafSize=self.getLeafSize())
        return m.set("ballTree", bt)


class ConditionalKNNModel(Model, _KNNParams, HasLabelCol):
    conditionerCol = Param("column holding identifiers for features that will be returned when queried",
                           "conditioner", T.toString)
    ballTree = Param("the ballTree model used for performing queries", None, complex=True)

    def _transform(self, df):
        bt: ConditionalBallTree = self.getBallTree()
        Q = as_matrix(df[self.getFeaturesCol()])
        conds = [set(c) for c in df[self.getConditionerCol()].tolist()]
        k = self.getK()
        res = []
        fused = _device_topk(bt, Q, k, conds) if _use_gpu() and len(Q) else None
        if fused is not None:
            vals, idx = fused
            for r in range(len(Q)):
                res.append([{"value": bt.values[int(i)], "distance": float(v), "label": bt.labels[int(i)]}
                            for v, i in zip(vals[r], idx[r]) if i >= 0])
        elif _use_gpu() and len(Q):
            labels = np.asarray(bt.labels, dtype=object)
            mask = np.stack([np.asarray([l in c for l in labels]) for c in conds])
            vals, idx = _device_mips(Q, bt.keys, k, mask)
            for r in range(len(Q)):
                res.append([{"value": bt.values[int(i)], "distance": float(v), "label": bt.labels[int(i)]}
                            for v, i in zip(vals[r], idx[r]) if np.isfinite(v)])
        else:
            for q, c in zip(Q, conds):
                res.append([{"value": bt.values[m.index], "distance": m.distance, "label": bt.labels[m.index]}
                            for m in bt.findMaximumInnerProducts(q, c, k)])
        return df.withColumn(self.getOutputCol(), _obj(res))


class ConditionalKNN(Estimator, _KNNParams, HasLabelCol):
    conditionerCol = Param("column holding identifiers for features that will be returned when queried",
                           "conditioner", T.toString)

    def __init__(self, **kw):
        super().__init__(**kw)
        self._setDefault(outputCol=self.uid + "_output")

    def _fit(self, df):
        bt = ConditionalBallTree(as_matrix(df[self.getFeaturesCol()]), df[self.getValuesCol()].tolist(),
                                 df[self.getLabelCol()].tolist(), self.getLeafSize())
        m = ConditionalKNNModel(featuresCol=self.getFeaturesCol(), valuesCol=self.getValuesCol(),
                                outputCol=self.getOutputCol(), k=self.getK(), leafSize=self.getLeafSize(),
                                labelCol=self.getLabelCol(), conditionerCol=self.getConditionerCol())
        return m.set("ballTree", bt)


__all__ = ["BallTree", "ConditionalBallTree", "BestMatch", "KNN", "KNNModel", "ConditionalKNN",
           "ConditionalKNNModel"]
