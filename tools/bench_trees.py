#!/usr/bin/env python3
"""Time the fused forest-walk kernel (K26, ops.trees) against the executor's torch walk (what ``SML_TREES=0``
runs) on the same resident device tensors, whole operator calls:

* a LightGBM-shaped binary classifier: 100 trees x 31 leaves (complete trees of 61 nodes), 28 features, one
  weight per leaf, LOGISTIC;
* a 10-class forest: 500 complete trees of depth 8 (511 nodes), 28 features, 10 weights per leaf, AVERAGE;

at batch sizes 1, 256, 65 536 and 1 048 576 (``--max-rows`` caps them). Both paths go through
``run_tree_ensemble``, alternating per repetition in one process, with device events around ``inner`` calls after
both were warmed at that shape; ``inner`` is chosen per path so that a window lasts about ``--window`` seconds.
The median and the min .. max over ``--reps`` are reported, and the launch shape the kernel path took. Bytes
are what the row-parallel kernel has to move: X once, the forest once per row tile, the leaf lists per reached
leaf, the outputs once; the bytes/s column is that over the call time. Kernel times come from a
``rocprofv3 --kernel-trace --stats`` run of this script with ``--reps 1 --window 0.05``. One JSON line per case,
a table at the end.

Usage: python tools/bench_trees.py [--reps 5] [--window 0.4] [--max-rows N] [--out LOG]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _events(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner  # us per call


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _forest(seed, T, nodes, F, K, per_leaf, **extra):
    """attributes of T complete binary trees in heap order (children of i are 2 i + 1, 2 i + 2)"""
    rng = np.random.default_rng(seed)
    i = np.tile(np.arange(nodes), T)
    leaf = 2 * i + 2 >= nodes
    at = {"nodes_treeids": np.repeat(np.arange(T), nodes).tolist(), "nodes_nodeids": i.tolist(),
          "nodes_featureids": np.where(leaf, 0, rng.integers(0, F, T * nodes)).tolist(),
          "nodes_values": np.where(leaf, 0, rng.standard_normal(T * nodes)).astype(np.float32).tolist(),
          "nodes_modes": np.where(leaf, "LEAF", "BRANCH_LEQ").tolist(),
          "nodes_truenodeids": np.where(leaf, 0, 2 * i + 1).tolist(),
          "nodes_falsenodeids": np.where(leaf, 0, 2 * i + 2).tolist(),
          "nodes_missing_value_tracks_true": rng.integers(0, 2, T * nodes).tolist()}
    lt, ln = np.repeat(np.arange(T), nodes)[leaf], i[leaf]
    at["class_treeids"] = np.repeat(lt, per_leaf).tolist()
    at["class_nodeids"] = np.repeat(ln, per_leaf).tolist()
    at["class_ids"] = np.tile(np.arange(per_leaf), len(lt)).tolist() if per_leaf > 1 else [0] * len(lt)
    at["class_weights"] = rng.standard_normal(len(lt) * per_leaf).astype(np.float32).tolist()
    at["classlabels_int64s"] = list(range(max(K, 2)))
    return {**at, **extra}, T * nodes, int(leaf.sum()) // T


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--max-rows", type=int, default=1 << 20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r12" / "trees" / "bench_trees.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trees: no GPU (nothing is measured without one)")
    from synapseml_amd.onnx.tree_ensemble import run_tree_ensemble
    from synapseml_amd.ops import native, trees

    rt = SimpleNamespace(op_type="TreeEnsembleClassifier")
    F = 28
    forests = [("lightgbm 100x31 binary", *_forest(0, 100, 61, F, 1, 1, post_transform="LOGISTIC"), 1, 1),
               ("forest 500xd8 10-class", *_forest(1, 500, 511, F, 10, 10, aggregate_function="AVERAGE"), 10, 10)]
    rows = []
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as log:
        def emit(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        emit(f"# bench_trees reps={a.reps} window={a.window} device={torch.cuda.get_device_name(0)}")
        for name, at, M, _, K, per_leaf in forests:
            T = len(set(at["nodes_treeids"]))
            for n in (1, 256, 1 << 16, 1 << 20):
                if n > a.max_rows:
                    continue
                X = torch.randn(n, F, generator=torch.Generator().manual_seed(n)).cuda()

                def run(flag, X=X, at=at):
                    os.environ["SML_TREES"] = flag
                    return run_tree_ensemble(rt, at, [X])

                fused, torch_ = (lambda: run("1")), (lambda: run("0"))
                try:
                    diff = float((fused()[1] - torch_()[1]).abs().max())  # the warm-up calls
                    labels_differ = int((fused()[0] != torch_()[0]).sum())
                except torch.OutOfMemoryError:
                    emit(json.dumps({"case": name, "n": n, "skipped": "the torch path cannot allocate this batch"}))
                    torch.cuda.empty_cache()
                    continue
                torch.cuda.synchronize()
                inner = [max(1, min(20000,int(a.window * 1e6 / _events(f, 3)))) for f in (fused, torch_)]
                tf, tt = [], []
                for _ in range(a.reps):
                    tf.append(_events(fused, inner[0]))
                    tt.append(_events(torch_, inner[1]))
                shape, slices = native.load("_nn").forest_plan(n, F, T, K, 0)
                tiles = (n + trees.ROW_TILE - 1) // trees.ROW_TILE
                nbytes = n * F * 4 + tiles * M * 16 + (n * T * per_leaf * 8 if per_leaf > 1 else 0) + n * (max(K, 2) * 4 + 8)
                row = {"case": name, "n": n, "launch": {1: "rows", 2: "trees"}[shape], "slices": slices,
                       "inner": inner, "bytes": nbytes, "fused_us": _median(tf), "fused_min_us": min(tf),
                       "fused_max_us": max(tf), "torch_us": _median(tt), "torch_min_us": min(tt),
                       "torch_max_us": max(tt), "max_abs_diff": diff, "labels_differ": labels_differ}
                row["fused_gbs"] = nbytes / row["fused_us"] / 1e3
                row["speedup"] = row["torch_us"] / row["fused_us"]
                rows.append(row)
                emit(json.dumps(row))
                del X
                torch.cuda.empty_cache()
        os.environ.pop("SML_TREES", None)
        # the two launch shapes against each other (the kernel entry alone), for the routing threshold
        for name, at, M, _, K, per_leaf in forests:
            forest = trees.pack(at, True)
            for n in (256, 2048, 16384, 1 << 16):
                X = torch.randn(n, F, generator=torch.Generator().manual_seed(n)).cuda()
                t = {}
                for launch in ("rows", "trees"):
                    fn = lambda: trees.tree_ensemble(X, forest, launch)  # noqa: E731
                    inner = max(1, min(20000,int(a.window * 1e6 / _events(fn, 3))))
                    t[launch] = _median([_events(fn, inner) for _ in range(a.reps)])
                emit(json.dumps({"routing": name, "n": n, "rows_us": t["rows"], "trees_us": t["trees"]}))
        emit(f"{'case':24s} {'n':>8s} {'launch':>6s} {'fused us':>26s} {'GB/s':>7s} {'torch us':>30s} {'speed-up':>8s}")
        for r in rows:
            emit(f"{r['case']:24s} {r['n']:8d} {r['launch']:>6s} {r['fused_us']:10.1f} ({r['fused_min_us']:.1f}.."
                 f"{r['fused_max_us']:.1f}) {r['fused_gbs']:7.1f} {r['torch_us']:12.1f} ({r['torch_min_us']:.1f}.."
                 f"{r['torch_max_us']:.1f}) {r['speedup']:8.2f}")
        slower = [f"{r['case']} n={r['n']}" for r in rows if r["fused_min_us"] > r["torch_max_us"]]
        emit(f"# fused slower than the torch path beyond the spread at: {slower if slower else 'no case'}")


if __name__ == "__main__":
    main()
