"""Python entry to the fused forest-walk kernel (K26, csrc/nn/forest_walk.hip): the ai.onnx.ml
TreeEnsembleClassifier / TreeEnsembleRegressor operators of the ONNX executor. ``pack`` turns the operator's
attribute lists into the kernel's forest once, on the host with numpy: 16-byte node records laid out tree by
tree, leaf payloads inline or in a list, per-tree offsets and depths, and the chunks of whole trees the
row-parallel kernel streams through LDS. ``tree_ensemble`` launches on the current stream with workspace from
torch's allocator; ``supported`` answers from shapes, dtypes, strides and devices alone. Nothing here reads a
tensor value, so the operator captures into a graph."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import native

MODES = {"BRANCH_LEQ": 0, "BRANCH_LT": 1, "BRANCH_GTE": 2, "BRANCH_GT": 3, "BRANCH_EQ": 4, "BRANCH_NEQ": 5, "LEAF": 6}
POSTS = {"NONE": 0, "LOGISTIC": 1, "SOFTMAX": 2}
LAUNCH = {"auto": 0, "rows": 1, "trees": 2}
CHUNK_NODES = 1024     # nodes of the LDS forest buffer (kForestChunkNodes)
ROW_TILE = 256         # rows of the largest row-parallel tile
REG_K = 8              # largest K whose scores stay in registers (kForestRegK)
MAX_LDS_F = 191        # widest X the row-parallel kernel stages in LDS (64-row tile, 48 KB); wider rows are read
                       # from global memory
MAX_K = 192            # the accumulator slab of a 64-row tile
MAX_TREE_NODES = 1 << 16   # child indices are 16 bits, relative to the tree
_MAX_ENTRIES = 1 << 28     # entries of one leaf (28 bits of the record)


@dataclass
class PackedForest:
    nodes: np.ndarray        # uint32 [M, 4]
    entries: np.ndarray      # uint32 [E, 2]: (id, weight bits) of the leaves with several entries
    tree_off: np.ndarray     # int32 [T + 1]
    tree_depth: np.ndarray   # int32 [T]
    chunk_tree: np.ndarray   # int32 [C + 1]
    K: int
    feat_min: int
    feat_max: int
    classifier: bool
    binary: bool
    average: bool
    post: int
    base: Optional[np.ndarray]          # fp32 [K]
    labels: Optional[list]              # class labels (ints or strings)
    _dev: dict = field(default_factory=dict, repr=False)

    @property
    def T(self) -> int:
        return len(self.tree_depth)

    def on(self, dev: torch.device) -> dict:
        """the forest's device tensors on dev, uploaded once"""
        d = self._dev.get(dev)
        if d is None:
            def up(a):
                return torch.from_numpy(a).to(dev)

            d = {"nodes": up(self.nodes.view(np.int32)), "tree_off": up(self.tree_off),
                 "tree_depth": up(self.tree_depth), "chunk_tree": up(self.chunk_tree),
                 "entries": up(self.entries.view(np.int32)) if len(self.entries) else None,
                 "base": None if self.base is None else up(self.base),
                 "labels": (up(np.asarray([int(v) for v in self.labels], np.int64))
                            if self.labels and not isinstance(self.labels[0], str) else None)}
            self._dev[dev] = d
        return d


def _tree_depths(tree_of, tchild, fchild, branch, roots, T, limit):
    """longest root-to-leaf path of every tree, walked level by level over all trees at once; a cyclic tree
    stops at its node count"""
    depth = np.zeros(T, np.int32)
    front = np.zeros(len(tree_of), bool)
    front[roots] = True
    for level in range(1, limit + 1):
        src = np.nonzero(front & branch)[0]
        if not len(src):
            break
        front[:] = False
        front[tchild[src]] = True
        front[fchild[src]] = True
        depth[tree_of[src]] = level
    return depth


def pack(at: dict, classifier: bool) -> Optional[PackedForest]:
    """The packed forest of a TreeEnsemble node's attributes, or None where the kernel does not serve them
    (the caller keeps its own path): the ``*_as_tensor`` double attributes, a post-transform other than NONE /
    LOGISTIC / SOFTMAX (SOFTMAX on a regressor included), duplicate or negative node ids, weights that name a
    missing node or an id outside [0, K), fewer class labels than scores, base values that are not one per score, a tree of more than
    MAX_TREE_NODES nodes, more than MAX_K scores."""
    if any(k.endswith("_as_tensor") and at[k] is not None for k in at):
        return None
    post = POSTS.get(at.get("post_transform", "NONE"))
    if post is None or (post == 2 and not classifier):
        return None
    tids = np.asarray(at.get("nodes_treeids", []), np.int64)
    nids = np.asarray(at.get("nodes_nodeids", []), np.int64)
    m = len(tids)
    if not m or len(nids) != m or nids.min() < 0:
        return None
    feat = np.asarray(at.get("nodes_featureids", [0] * m), np.int64)
    vals = np.asarray(at.get("nodes_values", [0.0] * m), np.float32)
    names = at.get("nodes_modes", ["LEAF"] * m)
    if any(s not in MODES for s in names):
        return None
    modes = np.asarray([MODES[s] for s in names], np.int64)
    tn = np.asarray(at.get("nodes_truenodeids", [0] * m), np.int64)
    fn = np.asarray(at.get("nodes_falsenodeids", [0] * m), np.int64)
    miss = np.asarray(at.get("nodes_missing_value_tracks_true", [0] * m), np.int64) != 0
    if not all(len(a) == m for a in (feat, vals, modes, tn, fn, miss)):
        return None
    trees, trank = np.unique(tids, return_inverse=True)
    T, span = len(trees), int(nids.max()) + 1
    if T * span >= 1 << 62:
        return None
    comb = trank * span + nids
    by_key = np.argsort(comb, kind="stable")
    keys = comb[by_key]
    if (keys[1:] == keys[:-1]).any():
        return None

    def find(rank, node):
        """index of node (rank, node id) in the attribute lists, -1 where there is none"""
        ok = (node >= 0) & (node < span)
        pos = np.minimum(np.searchsorted(keys, rank * span + np.where(ok, node, 0)), m - 1)
        return np.where(ok & (keys[pos] == rank * span + node), by_key[pos], -1)

    me = np.arange(m)
    leaf = modes == 6
    tchild, fchild = find(trank, tn), find(trank, fn)
    tchild = np.where(leaf | (tchild < 0), me, tchild)   # a leaf, or a child that does not exist: stay
    fchild = np.where(leaf | (fchild < 0), me, fchild)
    roots = find(np.arange(T), np.zeros(T, np.int64))
    first = np.full(T, m, np.int64)
    np.minimum.at(first, trank, me)
    roots = np.where(roots < 0, first, roots)
    is_root = np.zeros(m, bool)
    is_root[roots] = True
    order = np.lexsort((me, ~is_root, trank))             # tree by tree, the root first
    newpos = np.empty(m, np.int64)
    newpos[order] = me
    counts = np.bincount(trank, minlength=T)
    if counts.max() > MAX_TREE_NODES:
        return None
    tree_off = np.zeros(T + 1, np.int64)
    np.cumsum(counts, out=tree_off[1:])
    rel_t = newpos[tchild] - tree_off[trank]
    rel_f = newpos[fchild] - tree_off[trank]
    assert rel_t.min() >= 0 and rel_f.min() >= 0 and (rel_t < counts[trank]).all() and (rel_f < counts[trank]).all()

    pfx = "class_" if classifier else "target_"
    ct = np.asarray(at.get(pfx + "treeids", []), np.int64)
    cn = np.asarray(at.get(pfx + "nodeids", []), np.int64)
    cid = np.asarray(at.get(pfx + "ids", []), np.int64)
    cw = np.asarray(at.get(pfx + "weights", []), np.float32)
    if not len(ct) == len(cn) == len(cid) == len(cw):
        return None
    labels = None
    if classifier:
        labels = at.get("classlabels_int64s") or at.get("classlabels_strings")
        if not labels:
            return None
        K = max(int(cid.max()) + 1 if len(cid) else 1, 1)
    else:
        K = int(at.get("n_targets", 1))
    if not 0 < K <= MAX_K or (len(cid) and (cid.min() < 0 or cid.max() >= K)) or (classifier and len(labels) < K):
        return None
    crank = np.searchsorted(trees, ct)
    known = (crank < T) & (trees[np.minimum(crank, T - 1)] == ct)
    owner = find(np.where(known, crank, 0), cn)
    if not known.all() or (owner < 0).any():
        return None
    keep = leaf[owner]                                    # weights on a branch node are never reached
    owner, cid, cw = newpos[owner[keep]], cid[keep], cw[keep]
    by_leaf = np.argsort(owner, kind="stable")            # a leaf's entries keep their order
    owner, cid, cw = owner[by_leaf], cid[by_leaf], cw[by_leaf]
    cnt = np.bincount(owner, minlength=m)
    if cnt.max(initial=0) >= _MAX_ENTRIES:
        return None
    several = cnt[owner] > 1
    begin = np.zeros(m, np.int64)
    begin[cnt > 1] = np.cumsum(cnt[cnt > 1]) - cnt[cnt > 1]
    entries = np.stack([cid[several].astype(np.uint32), cw[several].view(np.uint32)], 1) if several.any() \
        else np.zeros((0, 2), np.uint32)
    if len(entries) >= 1 << 31:
        return None

    rec = np.zeros((m, 4), np.uint32)
    o = order
    rec[:, 0] = vals[o].view(np.uint32)
    rec[:, 1] = np.where(leaf[o], 0, np.clip(feat[o], 0, (1 << 32) - 1)).astype(np.uint32)
    rec[:, 2] = (modes[o] | (miss[o].astype(np.int64) << 3) | (cnt << 4)).astype(np.uint32)
    rec[:, 3] = np.where(leaf[o], 0, rel_t[o] | (rel_f[o] << 16)).astype(np.uint32)
    single = ~several                                     # one entry: the payload sits in the record
    rec[owner[single], 0] = cw[single].view(np.uint32)
    rec[owner[single], 1] = cid[single].astype(np.uint32)
    rec[cnt > 1, 1] = begin[cnt > 1].astype(np.uint32)

    depth = _tree_depths(trank, tchild, fchild, ~leaf, roots, T, int(counts.max()))
    chunk_tree, used = [0], 0
    for t in range(T):
        if used and used + counts[t] > CHUNK_NODES:
            chunk_tree.append(t)
            used = 0
        used += int(counts[t])
    chunk_tree.append(T)
    base = at.get("base_values")
    if base and len(base) != K:
        return None
    return PackedForest(
        nodes=rec, entries=np.ascontiguousarray(entries), tree_off=tree_off.astype(np.int32), tree_depth=depth,
        chunk_tree=np.asarray(chunk_tree, np.int32), K=K, feat_min=int(feat.min()), feat_max=int(feat.max()),
        classifier=classifier, binary=bool(classifier and len(labels) == 2 and K == 1),
        average=at.get("aggregate_function", "SUM") == "AVERAGE", post=post,
        base=np.asarray(base, np.float32) if base else None, labels=list(labels) if classifier else None)


def supported(X, forest: Optional[PackedForest]) -> bool:
    """Whether the kernel takes X [n, F] with this forest. Declined (the caller keeps its own path): no packed
    forest (see pack()), host tensors, anything but a non-empty 2-D fp32 tensor with unit inner stride."""
    return (forest is not None and isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32
            and X.dim() == 2 and X.numel() > 0 and (X.shape[1] == 1 or X.stride(1) == 1) and X.stride(0) >= 0)


def tree_ensemble(X: torch.Tensor, forest: PackedForest, launch: str = "auto"):
    """(out, label) of the ensemble on the rows of X. out is fp32 [n, K] (a classifier with two labels and one
    score column: [n, 2]); label is None for a regressor, else int64 [n]: the class labels, or the class
    indices where the labels are strings. ``launch``: "auto" routes by batch size, "rows" / "trees" force the
    row-parallel / tree-parallel kernel. Raises ValueError when a node's feature id is outside X's columns."""
    if forest is not None and isinstance(X, torch.Tensor) and X.dim() == 2 and \
            (forest.feat_max >= X.shape[1] or forest.feat_min < 0):
        raise ValueError(f"tree_ensemble: feature id {forest.feat_max if forest.feat_min >= 0 else forest.feat_min} "
                         f"is outside the {X.shape[1]} columns of X")
    if not supported(X, forest):
        raise ValueError("tree_ensemble: operands not supported (see supported())")
    n, F = X.shape
    K, dev = forest.K, X.device
    d = forest.on(dev)
    nn = native.load("_nn")
    with torch.cuda.device(dev):  # the plan and the launch size their grids for the current device
        shape, slices = nn.forest_plan(n, F, forest.T, K, LAUNCH[launch])
        if shape < 0:
            raise RuntimeError(f"tree_ensemble: launch {launch!r} does not take n={n} F={F} T={forest.T} K={K}")
        out = torch.empty((n, 2 if forest.binary else K), device=dev, dtype=torch.float32)
        label = torch.empty(n, device=dev, dtype=torch.int64) if forest.classifier else None
        ws = torch.empty(slices * n * K, device=dev, dtype=torch.float32) if slices else None

        def ptr(t):
            return 0 if t is None else t.data_ptr()

        took = nn.forest_walk(
            [X.data_ptr(), ptr(d["nodes"]), ptr(d["entries"]), ptr(d["tree_off"]), ptr(d["tree_depth"]),
             ptr(d["chunk_tree"]), ptr(d["base"]), out.data_ptr(), ptr(label), ptr(d["labels"]), ptr(ws)],
            [n, F, X.stride(0) if n > 1 else F, forest.T, len(forest.chunk_tree) - 1, K, int(forest.average),
             forest.post, int(forest.binary), int(forest.classifier), LAUNCH[launch], slices * n * K],
            torch.cuda.current_stream(dev).cuda_stream)
    if not took:
        raise RuntimeError("tree_ensemble: not taken by the kernel (check supported() first)")
    return out, label
