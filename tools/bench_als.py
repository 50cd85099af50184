#!/usr/bin/env python3
"""Time the fused sparse ALS half-sweep kernel (K27, ops.als) and ``ALS.fit`` on it against the dense body (what
``SML_ALS=0`` runs), on seeded rating sets:

* ``uniform``: 8192 x 8192 at 1 % density;
* ``ml20m``: 138 493 x 26 744 with 20 M draws from a power law over users and items;
* ``big`` (``--big``): 1 M x 100 k with 100 M draws, sparse path alone;

(duplicate pairs of the draws are dropped, so both paths see one rating per pair)

at ranks 10 and 64, explicit and implicit. Per case: the host preparation (``ops.als.prepare``) on a host clock;
one half-sweep of each side alone, device events around ``inner`` calls after a warm-up; and ``ALS.fit`` with
``--iters`` sweeps on both paths, alternating per repetition in one process, on a host clock (fit ends in a
device-to-host copy). The dense body is skipped where its matrices do not fit (``--dense-gb``) or the allocator
gives up. Bytes of a half-sweep are what the kernel has to gather: nnz factor rows of kp doubles plus the CSR
payload; flops are the 2 * 16 * 16 * 4 of every matrix instruction issued. One JSON line per case.

Usage: python tools/bench_als.py [--reps 3] [--iters 2] [--cases uniform,ml20m] [--big] [--no-fit]
       [--seg-len L] [--out LOG]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _ratings(name):
    rng = np.random.default_rng(0)
    if name == "uniform":
        nU = nI = 8192
        n = nU * nI // 100
        u, i = rng.integers(0, nU, n), rng.integers(0, nI, n)
    else:
        nU, nI, n = (138493, 26744, 20_000_000) if name == "ml20m" else (1_000_000, 100_000, 100_000_000)
        u = (nU * rng.random(n) ** 1.5).astype(np.int64)
        i = (nI * rng.random(n) ** 2.0).astype(np.int64)
    u[0], i[0] = nU - 1, nI - 1  # the shape ALS.fit reads from the largest ids
    _, first = np.unique(u * nI + i, return_index=True)  # one rating per pair: the dense scatter on the device
    u, i = u[first], i[first]                            # keeps an arbitrary one of a pair's duplicates
    return u, i, rng.integers(1, 6, len(u)).astype(np.float64), nU, nI


def _sweep_us(als, prep, side, X, Y, implicit, window):
    def run(inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            als.half_sweep(prep, side, X, Y, 0.1, 1.0, implicit, False)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / inner

    inner = max(1, min(1000, int(window * 1e6 / run(2))))
    return _median([run(inner) for _ in range(3)])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--cases", default="uniform,ml20m")
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--dense-gb", type=float, default=200.0)
    ap.add_argument("--no-fit", action="store_true", help="half-sweeps only (kernel traces, tuning)")
    ap.add_argument("--seg-len", type=int, default=0, help="try another segment length L")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13" / "als" / "bench_als.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_als: no GPU (nothing is measured without one)")
    from synapseml_amd.core import DataFrame
    from synapseml_amd.ops import als
    from synapseml_amd.recommendation import ALS

    if a.seg_len:
        als.L = a.seg_len
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as log:
        def emit(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        emit(f"# bench_als reps={a.reps} iters={a.iters} L={als.L} device={torch.cuda.get_device_name(0)}")
        for name in [c for c in a.cases.split(",") if c] + (["big"] if a.big and "big" not in a.cases else []):
            u, i, r, nU, nI = _ratings(name)
            t0 = time.perf_counter()
            prep = als.prepare(u, i, r, nU, nI)
            prep_s = time.perf_counter() - t0
            nnz = len(prep.sides[0].indices)
            emit(json.dumps({"case": name, "nU": nU, "nI": nI, "nnz": nnz, "prepare_s": prep_s,
                             "longest_rows": [int(s.tasks[0, 2]) if not len(s.red) else int(s.red[:, 3].max())
                                              for s in prep.sides], "cut_rows": [len(s.red) for s in prep.sides]}))
            df = DataFrame({"user": u.astype(np.float64), "item": i.astype(np.float64), "rating": r})
            for k in (10, 64):
                kp = als.padded_rank(k)
                for implicit in (False, True):
                    g = torch.Generator().manual_seed(0)
                    U = als.factors(torch.rand(nU, k, generator=g, dtype=torch.float64) * 0.1, "cuda")
                    V = als.factors(torch.rand(nI, k, generator=g, dtype=torch.float64) * 0.1, "cuda")
                    row = {"case": name, "rank": k, "implicit": implicit}
                    for side, X, Y in ((0, U, V), (1, V, U)):
                        us = _sweep_us(als, prep, side, X, Y, implicit, a.window)
                        nbytes = nnz * (kp * 8 + 12)
                        steps = int(((prep.sides[side].tasks[:, 2] + 3) // 4).sum())
                        flops = steps * (kp // 16) * (kp // 16 + 1) // 2 * 2 * 16 * 16 * 4
                        row[f"sweep{side}_us"] = us
                        row[f"sweep{side}_gather_gbs"] = nbytes / us / 1e3
                        row[f"sweep{side}_mfma_tflops"] = flops / us / 1e6
                    del U, V
                    if a.no_fit:
                        emit(json.dumps(row))
                        continue
                    dense_gb = nU * nI * 8 * (7 if implicit else 4) / 1e9
                    est = ALS(rank=k, maxIter=a.iters, implicitPrefs=implicit)

                    def fit(flag):
                        os.environ["SML_ALS"] = flag
                        t = time.perf_counter()
                        m = est.fit(df)
                        return time.perf_counter() - t, m

                    dense = name != "big" and dense_gb <= a.dense_gb
                    ts, td, diff = [], [], None
                    try:
                        _, ms = fit("1")  # the warm-up fits
                        if dense:
                            _, md = fit("0")
                            diff = float(max(np.abs(ms.getUserFactors() - md.getUserFactors()).max(),
                                             np.abs(ms.getItemFactors() - md.getItemFactors()).max()))
                            del md
                        for _ in range(a.reps):
                            ts.append(fit("1")[0])
                            if dense:
                                td.append(fit("0")[0])
                    except torch.OutOfMemoryError:
                        row["dense_skipped"] = "the dense body cannot allocate this shape"
                        td = []
                    torch.cuda.empty_cache()
                    if not dense:
                        row["dense_skipped"] = f"dense matrices of about {dense_gb:.0f} GB"
                    row.update({"fit_sparse_s": _median(ts) if ts else None, "fit_sparse_min_max": [min(ts), max(ts)]
                                if ts else None})
                    if td:
                        row.update({"fit_dense_s": _median(td), "fit_dense_min_max": [min(td), max(td)],
                                    "fit_speedup": _median(td) / _median(ts), "max_abs_diff": diff})
                    emit(json.dumps(row))
            del prep, df
            torch.cuda.empty_cache()
        os.environ.pop("SML_ALS", None)


if __name__ == "__main__":
    main()
