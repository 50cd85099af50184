#!/usr/bin/env python3
"""Time the fused MFMA top-k inner-product search (K23, ops.mips) against the torch path of the nearest-neighbour
stages on the same resident fp32 device tensors: the device steps of ``nn._device_mips`` (``q @ K.T``, the
conditioner's ``masked_fill``, ``torch.topk``) per 8192-query block, without its upload and download. Shapes:
N in {100k, 1M} keys, D in {16, 128, 2048}, k in {5, 50}, M = 64 queries (the key-split path) and 8192; a
conditional case with 64 labels and conditioner sets of 1 and 8 labels, for which ``ConditionalKNNModel.transform``
is also timed end to end (host clock, upload and host mask included) against ``SML_MIPS=0``.

Both paths are timed in one process, alternating per repetition, with device events around ``inner`` calls (sized
from one timed call so that a repetition lasts about ``--budget`` seconds) after a warm-up of every shape; the
median and the min .. max over ``--reps`` are reported. FLOP/s is 2 M N D / time. The binding limit named per
shape is the larger of the fp32 MFMA time (2 M N D over the peak rate, D rounded up to 16) and the key bytes
over the HBM rate (per resident query wave). One JSON line per shape, a table at the end.

Usage: python tools/bench_mips.py [--reps 5] [--budget 0.3] [--out LOG]
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

PEAK_F32_MFMA = 157.3e12  # MI355X fp32 matrix FLOP/s (data sheet)
PEAK_HBM = 8.0e12         # bytes/s

# (M, N, D, k, labels, conditioner set size)
SHAPES = [(M, N, D, k, 0, 0) for N in (100_000, 1_000_000) for D in (16, 128, 2048) for M in (64, 8192) for k in (5, 50)]
SHAPES += [(8192, 100_000, 128, 5, 64, 1), (8192, 100_000, 128, 5, 64, 8)]


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


def _allow_bits(sets, labels):
    bits = np.zeros((len(sets), (labels + 31) // 32), np.uint32)
    for r, c in enumerate(sets):
        for l in c:
            bits[r, l >> 5] |= np.uint32(1 << (l & 31))
    return bits.view(np.int32)


def _end_to_end(emit, labels, set_size, rng):
    """ConditionalKNNModel.transform, host clock: the fused path against SML_MIPS=0 (host mask + _device_mips)"""
    from synapseml_amd import nn
    from synapseml_amd.core.dataframe import DataFrame

    N, D, Q, k = 100_000, 128, 256, 5
    bt = nn.ConditionalBallTree(rng.normal(size=(N, D)), list(range(N)), rng.integers(0, labels, N).tolist(),
                                leafSize=N)
    model = nn.ConditionalKNNModel(k=k, outputCol="matches").set("ballTree", bt)
    cond = np.empty(Q, dtype=object)
    for i in range(Q):
        cond[i] = rng.choice(labels, set_size, replace=False).tolist()
    df = DataFrame({"features": rng.normal(size=(Q, D)), "conditioner": cond})
    times = {"1": [], "0": []}
    for rep in range(4):  # repetition 0 is the warm-up (and the one upload of the keys on the fused path)
        for flag in ("1", "0"):
            os.environ["SML_MIPS"] = flag
            t0 = time.perf_counter()
            model.transform(df)
            torch.cuda.synchronize()
            if rep:
                times[flag].append((time.perf_counter() - t0) * 1e3)
    os.environ.pop("SML_MIPS", None)
    row = {"end_to_end": "ConditionalKNNModel.transform", "Q": Q, "N": N, "D": D, "k": k, "labels": labels,
           "set": set_size, "fused_ms": _median(times["1"]), "fused_min_ms": min(times["1"]),
           "fused_max_ms": max(times["1"]), "torch_ms": _median(times["0"]), "torch_min_ms": min(times["0"]),
           "torch_max_ms": max(times["0"])}
    emit(json.dumps(row))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r9" / "mips" / "bench_mips.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mips: no GPU (nothing is measured without one)")
    from synapseml_amd.ops import mips

    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    rows = []
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as log:
        def emit(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        emit(f"# bench_mips reps={a.reps} budget={a.budget}s device={torch.cuda.get_device_name(0)}")
        keys = None
        for M, N, D, k, labels, set_size in SHAPES:
            if keys is None or keys.shape != (N, D):
                keys = None
                keys = torch.randn(N, D, device="cuda", generator=gen)
            q = torch.randn(M, D, device="cuda", generator=gen)
            key_label = allow = mask = None
            if labels:
                lab = rng.integers(0, labels, N)
                sets = [rng.choice(labels, set_size, replace=False) for _ in range(M)]
                key_label = torch.as_tensor(lab.astype(np.int32), device="cuda")
                allow = torch.as_tensor(_allow_bits(sets, labels), device="cuda")
                member = np.zeros((M, labels), bool)
                for r, c in enumerate(sets):
                    member[r, c] = True
                mask = torch.as_tensor(member, device="cuda")[:, key_label.long()]
            fused = lambda: mips.topk(q, keys, k, key_label, allow)  # noqa: E731

            def torch_():
                sc = q @ keys.T
                if mask is not None:
                    sc = sc.masked_fill(~mask, float("-inf"))
                return torch.topk(sc, min(k, N), dim=1)

            diff = float((fused()[0] - torch_()[0]).abs().max())  # the warm-up calls
            torch.cuda.synchronize()
            inner_f = max(1, min(50, int(a.budget * 1e6 / _events(fused, 1))))
            inner_t = max(1, min(50, int(a.budget * 1e6 / _events(torch_, 1))))
            tf, tt = [], []
            for _ in range(a.reps):
                tf.append(_events(fused, inner_f))
                tt.append(_events(torch_, inner_t))
            flop = 2.0 * M * N * D
            waves = -(-M // (64 * 256))  # passes over the keys when the query tiles exceed the resident blocks
            t_mfma = 2.0 * M * N * (-(-D // 16) * 16) / PEAK_F32_MFMA
            t_keys = 4.0 * N * D * waves / PEAK_HBM
            row = {"M": M, "N": N, "D": D, "k": k, "labels": labels, "set": set_size,
                   "splits": mips.plan_splits(M, N, k, bool(labels)), "fused_us": _median(tf), "fused_min_us": min(tf),
                   "fused_max_us": max(tf), "torch_us": _median(tt), "torch_min_us": min(tt), "torch_max_us": max(tt),
                   "max_abs_diff": diff, "bound": "fp32 MFMA rate" if t_mfma >= t_keys else "key bytes",
                   "bound_us": max(t_mfma, t_keys) * 1e6}
            row["fused_tflops"] = flop / row["fused_us"] / 1e6
            row["speedup"] = row["torch_us"] / row["fused_us"]
            rows.append(row)
            emit(json.dumps(row))
        keys = None
        for set_size in (1, 8):
            _end_to_end(emit, 64, set_size, rng)
        emit(f"{'M':>5s} {'N':>8s} {'D':>5s} {'k':>3s} {'cond':>5s} {'fused us':>30s} {'torch us':>30s} {'TFLOP/s':>8s} "
             f"{'speed-up':>8s}  bound")
        for r in rows:
            emit(f"{r['M']:5d} {r['N']:8d} {r['D']:5d} {r['k']:3d} {r['labels']:2d}/{r['set']:<2d} "
                 f"{r['fused_us']:12.1f} ({r['fused_min_us']:.1f}..{r['fused_max_us']:.1f})"
                 f" {r['torch_us']:12.1f} ({r['torch_min_us']:.1f}..{r['torch_max_us']:.1f})"
                 f" {r['fused_tflops']:8.2f} {r['speedup']:8.2f}  {r['bound']} ({r['bound_us']:.0f} us)")
        slower = [f"M{r['M']} N{r['N']} D{r['D']} k{r['k']} cond {r['labels']}/{r['set']}" for r in rows
                  if r["fused_min_us"] > r["torch_max_us"]]
        faster = sum(r["fused_max_us"] < r["torch_min_us"] for r in rows)
        emit(f"# fused faster beyond the spread at {faster} of {len(rows)} shapes; slower beyond the spread at: "
             f"{slower if slower else 'no shape'}")


if __name__ == "__main__":
    main()
