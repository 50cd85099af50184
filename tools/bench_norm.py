#!/usr/bin/env python3
"""Time the fused row-normalisation and bias-activation kernels (K25, ops.norm) against the executor's torch
bodies (what ``SML_NORM=0`` runs) on the same resident device tensors, fp16 and fp32 (bias-GELU also bf16):

* skip layer norm with bias and sum output, plain layer norm and RMS norm at 12288 x 768 and 12288 x 1024
  (BERT-base / -large at S = 384, batch 32), and at 4096 x 4096 (the block-per-row form);
* bias-GELU at 12288 x 3072 and 12288 x 4096;
* embed layer norm at batch 32, S = 384 over a 30522 x 1024 vocabulary.

Both paths go through the operator functions of the executor, so a time is that of an operator call in a stream
of such calls: the kernel, or the Python that enqueues it where that takes longer (the small norms). Kernel
times come from a ``rocprofv3 --kernel-trace --stats`` run of this script with few repetitions.
They are timed in one process, alternating per repetition, with device events around ``--inner`` calls after a
warm-up of every shape; the median and the min .. max over ``--reps`` are reported. Bytes are what the fused
operator has to move (every input read once, every output written once), so the bytes/s of the torch path is
the same traffic over its time, not what it really moved. One JSON line per case, a table at the end.

Usage: python tools/bench_norm.py [--reps 7] [--inner 1000] [--out LOG]
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

EPS = 1e-5


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


def _cases(dtype, gen):
    """(name, operator, inputs, attributes, outputs, bytes moved)"""
    from synapseml_amd.onnx.ops import OPS

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to("cuda", dtype)

    es = torch.empty((), dtype=dtype).element_size()
    for rows, N in () if dtype == torch.bfloat16 else ((12288, 768), (12288, 1024), (4096, 4096)):
        x, skip, gamma, beta, bias = rnd(32, rows // 32, N), rnd(32, rows // 32, N), rnd(N), rnd(N), rnd(N)
        act = rows * N * es
        yield (f"skip-LN+bias+sum {rows}x{N}", OPS["SkipLayerNormalization"], [x, skip, gamma, beta, bias],
               {"epsilon": EPS}, 4, 4 * act + 8 * rows)
        yield f"LN {rows}x{N}", OPS["LayerNormalization"], [x, gamma, beta], {"epsilon": EPS}, 1, 2 * act
        yield f"RMS {rows}x{N}", OPS["SimplifiedLayerNormalization"], [x, gamma], {"epsilon": EPS}, 1, 2 * act
    for rows, N in ((12288, 3072), (12288, 4096)):
        yield f"bias-GELU {rows}x{N}", OPS["BiasGelu"], [rnd(rows, N), rnd(N)], {}, 1, 2 * rows * N * es
    if dtype == torch.bfloat16:
        return
    B, S, N, V = 32, 384, 1024, 30522
    ids = torch.randint(0, V, (B, S), generator=gen).cuda()
    seg_ids = torch.randint(0, 2, (B, S), generator=gen).cuda()
    yield (f"embed-LN {B}x{S} vocab {V}x{N}", OPS["EmbedLayerNormalization"],
           [ids, seg_ids, rnd(V, N), rnd(512, N), rnd(2, N), rnd(N), rnd(N)], {"epsilon": EPS}, 1,
           2 * B * S * N * es + 2 * B * S * 8)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=1000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r11" / "norm" / "bench_norm.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_norm: no GPU (nothing is measured without one)")
    import synapseml_amd.onnx.ops_ext  # noqa: F401  (registers the contrib operators)

    gen = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as log:
        def emit(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        emit(f"# bench_norm reps={a.reps} inner={a.inner} device={torch.cuda.get_device_name(0)}")
        for dtype in (torch.float16, torch.bfloat16, torch.float32):
            for name, fn, inputs, attrs, n_out, nbytes in _cases(dtype, gen):
                rt = SimpleNamespace(node_num_outputs=n_out)

                def run(flag, fn=fn, rt=rt, attrs=attrs, inputs=inputs):
                    os.environ["SML_NORM"] = flag
                    return fn(rt, attrs, inputs)

                fused, torch_ = (lambda: run("1")), (lambda: run("0"))
                diff = float((fused()[0].float() - torch_()[0].float()).abs().max())  # the warm-up calls
                torch.cuda.synchronize()
                tf, tt = [], []
                for _ in range(a.reps):
                    tf.append(_events(fused, a.inner))
                    tt.append(_events(torch_, a.inner))
                row = {"case": name, "dtype": str(dtype).split(".")[1], "bytes": nbytes, "fused_us": _median(tf),
                       "fused_min_us": min(tf), "fused_max_us": max(tf), "torch_us": _median(tt),
                       "torch_min_us": min(tt), "torch_max_us": max(tt), "max_abs_diff": diff}
                row["fused_gbs"] = nbytes / row["fused_us"] / 1e3
                row["torch_gbs"] = nbytes / row["torch_us"] / 1e3
                row["speedup"] = row["torch_us"] / row["fused_us"]
                rows.append(row)
                emit(json.dumps(row))
                del inputs
                torch.cuda.empty_cache()
        os.environ.pop("SML_NORM", None)
        emit(f"{'case':34s} {'dtype':>8s} {'fused us':>22s} {'GB/s':>7s} {'torch us':>24s} {'GB/s':>7s} {'speed-up':>8s}")
        for r in rows:
            emit(f"{r['case']:34s} {r['dtype']:>8s} {r['fused_us']:8.1f} ({r['fused_min_us']:.1f}..{r['fused_max_us']:.1f})"
                 f" {r['fused_gbs']:7.0f} {r['torch_us']:9.1f} ({r['torch_min_us']:.1f}..{r['torch_max_us']:.1f})"
                 f" {r['torch_gbs']:7.0f} {r['speedup']:8.2f}")
        slower = [f"{r['case']} {r['dtype']}" for r in rows if r["fused_min_us"] > r["torch_max_us"]]
        emit(f"# fused slower than the torch path beyond the spread at: {slower if slower else 'no case'}")


if __name__ == "__main__":
    main()
