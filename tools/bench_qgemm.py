#!/usr/bin/env python3
"""Time the int8 MFMA GEMM / conv (K18, ops.qgemm) on the QLinearConv shapes of ResNet-50 at batch 128 and
one FC-sized QLinearMatMul. Every shape is timed three ways in one process, alternating per repetition:

  q8    ops.qgemm.qlinear_conv / qlinear_matmul (the new kernel; the per-call weight pack included)
  f16   K17 fp16 on the same M, N, K (ops.conv.conv2d_nhwc_general / ops.gemm.gemm)
  host  the executor's operator with SML_QGEMM=0 (fp64 on the host, device -> host -> device)

q8 and f16 are timed with device events around ``--inner`` launches; host with a host clock around a call
that ends in a device synchronise. Every shape is warmed before it is timed. Operations (2 M N K) and bytes
(input + weight + output) come from the shapes. One JSON line per shape, a table at the end.

Usage: python tools/bench_qgemm.py [--batch 128] [--reps 5] [--inner 10] [--host-reps 1] [--out LOG]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

# ResNet-50 v1.5 convolutions other than the stem: (Cin, H = W of the input, Cout, R = S, stride)
RESNET50 = [
    (64, 56, 64, 1, 1), (64, 56, 64, 3, 1), (64, 56, 256, 1, 1), (256, 56, 64, 1, 1),
    (256, 56, 128, 1, 1), (128, 56, 128, 3, 2), (128, 28, 512, 1, 1), (256, 56, 512, 1, 2),
    (512, 28, 128, 1, 1), (128, 28, 128, 3, 1),
    (512, 28, 256, 1, 1), (256, 28, 256, 3, 2), (256, 14, 1024, 1, 1), (512, 28, 1024, 1, 2),
    (1024, 14, 256, 1, 1), (256, 14, 256, 3, 1),
    (1024, 14, 512, 1, 1), (512, 14, 512, 3, 2), (512, 7, 2048, 1, 1), (1024, 14, 2048, 1, 2),
    (2048, 7, 512, 1, 1), (512, 7, 512, 3, 1),
]
FC = (2048, 1000)  # K, N of the classifier at M = batch


def _events(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner  # us per call


def _host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _measure(name, M, N, K, q8, f16, host, a):
    os.environ.pop("SML_QGEMM", None)
    yq, _ = q8(), f16()
    equal = bool(torch.equal(yq, host()[0])) if a.host_reps else None  # the host path's warm-up call
    torch.cuda.synchronize()
    tq, tf, th = [], [], []
    for rep in range(a.reps):
        tq.append(_events(q8, a.inner))
        tf.append(_events(f16, a.inner))
        if rep < a.host_reps:
            th.append(_host_clock(host))
    ops = 2.0 * M * N * K
    row = {"shape": name, "M": M, "N": N, "K": K, "q8_us": _median(tq), "f16_us": _median(tf),
           "host_us": _median(th) if th else None, "q8_min_us": min(tq), "q8_max_us": max(tq),
           "f16_min_us": min(tf), "f16_max_us": max(tf), "ops": ops, "q8_bytes": M * K + N * K + M * N,
           "f16_bytes": 2 * (M * K + N * K + M * N), "equals_host": equal}
    row["q8_tops"] = ops / row["q8_us"] / 1e6
    row["f16_tflops"] = ops / row["f16_us"] / 1e6
    row["q8_vs_f16"] = row["f16_us"] / row["q8_us"]
    return row


def _with_host_path(fn):
    def run():
        os.environ["SML_QGEMM"] = "0"
        try:
            return fn()
        finally:
            os.environ.pop("SML_QGEMM", None)

    return run


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r7" / "qgemm" / "bench_qgemm.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qgemm: no GPU (nothing is measured without one)")
    from synapseml_amd.onnx import ops_ext
    from synapseml_amd.ops import conv as C, gemm as G, qgemm as Q

    dev = "cuda"
    gen = torch.Generator(device="cpu").manual_seed(0)
    u8 = lambda *s: torch.randint(0, 256, s, generator=gen, dtype=torch.uint8).to(dev)  # noqa: E731
    s8 = lambda *s: torch.randint(-128, 128, s, generator=gen, dtype=torch.int16).to(torch.int8).to(dev)  # noqa: E731
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)  # noqa: E731
    rows = []
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as log:
        def emit(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        emit(f"# bench_qgemm batch={a.batch} reps={a.reps} inner={a.inner} host_reps={a.host_reps} "
             f"device={torch.cuda.get_device_name(0)}")
        for cin, hw, cout, r, stride in RESNET50:
            pad = r // 2
            x = u8(a.batch, cin, hw, hw).contiguous(memory_format=torch.channels_last)
            w = s8(cout, cin, r, r)
            x_s, x_z, w_s, w_z = f32(0.02), u8(1).reshape(()), torch.rand(cout, device=dev) * 0.01 + 0.001, s8(cout)
            y_s, y_z = f32(0.5), u8(1).reshape(())
            bias = torch.randint(-1000, 1000, (cout,), generator=gen, dtype=torch.int32).to(dev)
            pads = (pad, pad, pad, pad)
            x16 = x.to(torch.float16).contiguous(memory_format=torch.channels_last)
            wp16 = C.pack_weight(w, torch.float16)
            at = {"kernel_shape": [r, r], "strides": [stride, stride], "pads": list(pads)}
            inputs = [x, x_s, x_z, w, w_s, w_z, y_s, y_z, bias]
            q8 = lambda: Q.qlinear_conv(x, x_s, x_z, w, w_s, w_z, y_s, y_z, bias, (stride, stride), pads)  # noqa: E731
            f16 = lambda: C.conv2d_nhwc_general(x16, wp16, r, r, (stride, stride), pads)  # noqa: E731
            host = _with_host_path(lambda: ops_ext.OPS["QLinearConv"](None, at, inputs))
            yq = q8()
            M, K = yq.shape[0] * yq.shape[2] * yq.shape[3], r * r * cin
            row = _measure(f"conv{r}x{r} {cin}->{cout} @{hw} s{stride}", M, cout, K, q8, f16, host, a)
            rows.append(row)
            emit(json.dumps(row))
        K, N = FC
        am, bm = u8(a.batch, K), s8(K, N)
        a_s, a_z, b_s, b_z, y_s, y_z = f32(0.02), u8(1).reshape(()), f32(0.005), s8(1).reshape(()), f32(0.5), u8(1).reshape(())
        a16, b16 = am.to(torch.float16), bm.to(torch.float16)
        inputs = [am, a_s, a_z, bm, b_s, b_z, y_s, y_z]
        q8 = lambda: Q.qlinear_matmul(*inputs)  # noqa: E731
        f16 = lambda: G.gemm(a16, b16)  # noqa: E731
        host = _with_host_path(lambda: ops_ext.OPS["QLinearMatMul"](None, {}, inputs))
        row = _measure(f"matmul {a.batch}x{K}x{N}", a.batch, N, K, q8, f16, host, a)
        rows.append(row)
        emit(json.dumps(row))
        emit(f"{'shape':34s} {'q8 us':>9s} {'f16 us':>9s} {'host us':>11s} {'q8 TOP/s':>9s} {'f16/q8':>7s}")
        for r_ in rows:
            h = f"{r_['host_us']:11.0f}" if r_["host_us"] is not None else f"{'-':>11s}"
            emit(f"{r_['shape']:34s} {r_['q8_us']:9.1f} {r_['f16_us']:9.1f} {h} {r_['q8_tops']:9.1f} {r_['q8_vs_f16']:7.2f}")
        tq, tf = sum(r_["q8_us"] for r_ in rows), sum(r_["f16_us"] for r_ in rows)
        emit(f"# sum over shapes: q8 {tq:.0f} us, f16 {tf:.0f} us, f16 / q8 {tf / tq:.2f}")
        slower = [r_["shape"] for r_ in rows if r_["q8_vs_f16"] < 1.0]
        emit(f"# q8 slower than f16 at: {slower if slower else 'no shape'}")


if __name__ == "__main__":
    main()
