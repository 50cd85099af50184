#!/usr/bin/env python3
"""Time the fused MFMA attention (K22, ops.attention) against the executor's unfused ``_attend()`` (fp32 matmul,
softmax, matmul through torch) on the same fp16 / bf16 device tensors: BERT-base (12 heads) and BERT-large (16
heads) encoder shapes at S = L in {128, 384, 512} with a batch that fills the device, a causal S = L = 1024 case
and a head-size-128 case. q, k, v are the ``torch.split`` views of one packed [B, S, 3 D] projection, as the
Attention operator sees them; both paths get the same right-padding key mask (the kernel as its [B, L] key term).

Both paths are timed in one process, alternating per repetition, with device events around ``--inner`` calls after
a warm-up of every shape; the median and the min .. max over ``--reps`` are reported. Operations (4 B H S L d,
halved when causal) come from the shapes. One JSON line per shape and dtype, a table at the end.

Usage: python tools/bench_attention.py [--reps 7] [--inner 100] [--out LOG]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

# (name, batch, heads, head size, S = L, causal)
SHAPES = [(f"bert-{n} S{s}", b, h, 64, s, False)
          for n, h in (("base", 12), ("large", 16)) for s, b in ((128, 64), (384, 32), (512, 16))]
SHAPES += [("causal S1024", 8, 16, 64, 1024, True), ("d128 S512", 16, 8, 128, 512, False)]


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r8" / "attention" / "bench_attention.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention: no GPU (nothing is measured without one)")
    from synapseml_amd.onnx.ops_ext import _attend
    from synapseml_amd.ops import attention as A

    gen = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as log:
        def emit(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        emit(f"# bench_attention reps={a.reps} inner={a.inner} device={torch.cuda.get_device_name(0)}")
        for name, B, H, d, S, causal in SHAPES:
            for dtype in (torch.float16, torch.bfloat16):
                D = H * d
                q, k, v = torch.split(torch.randn(B, S, 3 * D, generator=gen).to("cuda", dtype), D, -1)
                lens = torch.randint(S // 2, S + 1, (B, 1), generator=gen)
                key_add = torch.where(torch.arange(S).unsqueeze(0) < lens, 0.0, -10000.0).cuda()
                mask_add = key_add.reshape(B, 1, 1, S)
                fused = lambda: A.attention(q, k, v, H, key_add=key_add, causal=causal)  # noqa: E731
                torch_ = lambda: _attend(q, k, v, H, None, mask_add, causal)  # noqa: E731
                diff = float((fused().float() - torch_().float()).abs().max())  # the warm-up calls
                torch.cuda.synchronize()
                tf, tt = [], []
                for _ in range(a.reps):
                    tf.append(_events(fused, a.inner))
                    tt.append(_events(torch_, a.inner))
                ops = 4.0 * B * H * S * S * d * (0.5 if causal else 1.0)
                row = {"shape": name, "dtype": str(dtype).split(".")[1], "B": B, "heads": H, "d": d, "S": S,
                       "causal": causal, "fused_us": _median(tf), "fused_min_us": min(tf), "fused_max_us": max(tf),
                       "attend_us": _median(tt), "attend_min_us": min(tt), "attend_max_us": max(tt),
                       "max_abs_diff": diff}
                row["fused_tflops"] = ops / row["fused_us"] / 1e6
                row["speedup"] = row["attend_us"] / row["fused_us"]
                rows.append(row)
                emit(json.dumps(row))
        emit(f"{'shape':16s} {'dtype':>8s} {'fused us':>20s} {'_attend us':>24s} {'TFLOP/s':>8s} {'speed-up':>8s}")
        for r in rows:
            emit(f"{r['shape']:16s} {r['dtype']:>8s} {r['fused_us']:8.1f} ({r['fused_min_us']:.1f}..{r['fused_max_us']:.1f})"
                 f" {r['attend_us']:9.1f} ({r['attend_min_us']:.1f}..{r['attend_max_us']:.1f})"
                 f" {r['fused_tflops']:8.1f} {r['speedup']:8.2f}")
        slower = [f"{r['shape']} {r['dtype']}" for r in rows if r["fused_min_us"] > r["attend_max_us"]]
        emit(f"# fused slower than _attend() beyond the spread at: {slower if slower else 'no shape'}")


if __name__ == "__main__":
    main()
