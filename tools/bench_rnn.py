#!/usr/bin/env python3
"""Time the ONNX LSTM / GRU operators on the fused persistent MFMA kernel (K24, ops.rnn) against the executor's
unfused time loop (``SML_RNN=0``: about fifteen torch launches per step and direction) on the same fp32 device
tensors, at tagger / speech shapes: (T, N, I = H) = (128, 64, 256) bidirectional, (50, 10, 128), (512, 1, 512),
and (128, 256, 1024) for LSTM only (beyond ops.rnn.MAX_HIDDEN: routed to the time loop, "kernel": false, both
columns time the same path). Both sides are the whole operator: input projection, the recurrence, outputs
(the fused side includes the repacking of R). sequence_lens is absent, so neither side reads a value on the host.

Both paths are timed in one process, alternating per repetition, with device events around ``--inner`` calls after
a warm-up of every shape; the median and the min .. max over ``--reps`` are reported. The recurrent operations
(2 T N nd gates H^2) come from the shapes. One JSON line per shape and operator, a table at the end.

Usage: python tools/bench_rnn.py [--reps 5] [--inner 3] [--out LOG]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

# (T, N, I = H, directions, operators)
SHAPES = [(128, 64, 256, 2, ("LSTM", "GRU")), (50, 10, 128, 1, ("LSTM", "GRU")), (512, 1, 512, 1, ("LSTM", "GRU")),
          (128, 256, 1024, 1, ("LSTM",))]


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r10" / "rnn" / "bench_rnn.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnn: no GPU (nothing is measured without one)")
    from synapseml_amd.onnx import ops_ext
    from synapseml_amd.ops import rnn

    gen = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as log:
        def emit(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        emit(f"# bench_rnn reps={a.reps} inner={a.inner} device={torch.cuda.get_device_name(0)}")
        for T, N, H, nd, cells in SHAPES:
            for cell in cells:
                G = 4 if cell == "LSTM" else 3
                X = torch.randn(T, N, H, generator=gen).cuda()
                W, R = (torch.randn(nd, G * H, H, generator=gen).cuda() / H ** 0.5 for _ in range(2))
                B = torch.randn(nd, 2 * G * H, generator=gen).cuda() * 0.1
                kernel = rnn.supported(X, W, R, G, B, direction="bidirectional" if nd == 2 else "forward")
                rt = SimpleNamespace(node_num_outputs=3 if cell == "LSTM" else 2)
                at = {"hidden_size": H, "direction": "bidirectional" if nd == 2 else "forward"}
                run = ops_ext.OPS[cell]

                def call(switch):
                    os.environ["SML_RNN"] = switch
                    return run(rt, at, [X, W, R, B])

                diff = max(float((f - o).abs().max()) for f, o in zip(call("1"), call("0")))  # the warm-up calls
                torch.cuda.synchronize()
                tf, tt = [], []
                for _ in range(a.reps):
                    tf.append(_events(lambda: call("1"), a.inner))
                    tt.append(_events(lambda: call("0"), a.inner))
                row = {"op": cell, "kernel": kernel, "T": T, "N": N, "H": H, "nd": nd, "fused_us": _median(tf),
                       "fused_min_us": min(tf), "fused_max_us": max(tf), "loop_us": _median(tt), "loop_min_us": min(tt),
                       "loop_max_us": max(tt), "max_abs_diff": diff}
                row["fused_tflops"] = 2.0 * T * N * nd * G * H * H / row["fused_us"] / 1e6
                row["speedup"] = row["loop_us"] / row["fused_us"]
                rows.append(row)
                emit(json.dumps(row))
        emit(f"{'op':5s} {'T':>4s} {'N':>4s} {'H':>5s} {'nd':>2s} {'fused us':>28s} {'time loop us':>32s} "
             f"{'TFLOP/s':>8s} {'speed-up':>8s}")
        for r in rows:
            emit(f"{r['op']:5s} {r['T']:4d} {r['N']:4d} {r['H']:5d} {r['nd']:2d} {r['fused_us']:10.1f} "
                 f"({r['fused_min_us']:.1f}..{r['fused_max_us']:.1f}) {r['loop_us']:12.1f} "
                 f"({r['loop_min_us']:.1f}..{r['loop_max_us']:.1f}) {r['fused_tflops']:8.2f} {r['speedup']:8.2f}")
        slower = [f"{r['op']} T{r['T']} N{r['N']} H{r['H']}" for r in rows if r["fused_min_us"] > r["loop_max_us"]]
        emit(f"# fused slower than the time loop beyond the spread at: {slower if slower else 'no shape'}")
    os.environ.pop("SML_RNN", None)


if __name__ == "__main__":
    main()
