"""Python entry to the fused MFMA attention forward (K22, csrc/nn/attn_mfma.hip): com.microsoft ``Attention`` /
``MultiHeadAttention`` of the ONNX executor. Operands are torch CUDA tensors, fp16 or bf16; q, k and v are read in
place through their strides (the ``torch.split`` views of a packed QKV projection need no copy), launches go on
the current stream. Masks and biases stay on the device as additive fp32 terms the kernel reads: nothing here
reads a tensor value, so a launch never waits for the device and captures into a graph."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import native

_DT = {torch.float16: 1, torch.bfloat16: 2}
HEAD_SIZES = (32, 64, 128)  # compiled head sizes; 96 is declined
_MAX_GRID = 65535           # heads and batch are grid dimensions y and z
_MAX_SLICE = 1 << 30        # elements one (batch, head) slice may span: 32-bit byte offsets in the kernel


def _bias_ok(bias: torch.Tensor, B: int, heads: int, S: int, L: int) -> bool:
    if bias.dim() != 4 or not bias.is_cuda:
        return False
    return all(n in (1, full) for n, full in zip(bias.shape[:3], (B, heads, S))) and bias.shape[3] == L


def supported(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, key_add: Optional[torch.Tensor] = None,
              bias: Optional[torch.Tensor] = None, causal: bool = False) -> bool:
    """Whether the kernel takes this problem: q [B, S, D], k and v [B, L, D] on the device, all fp16 or all
    bf16, D / heads in HEAD_SIZES. Declined (the caller keeps its own path): host tensors, other or mixed
    dtypes, other head sizes, a v width different from q's, causal with L < S, empty tensors, batch or heads
    beyond the grid limits, ``key_add`` not [B, L], ``bias`` not broadcastable [B|1, heads|1, S|1, L]."""
    if not (q.is_cuda and k.is_cuda and v.is_cuda and q.dtype in _DT and k.dtype == q.dtype and v.dtype == q.dtype):
        return False
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or not (q.numel() and k.numel() and v.numel()):
        return False
    B, S, D = q.shape
    L = k.shape[1]
    if k.shape != (B, L, D) or v.shape != (B, L, D) or heads < 1 or D % heads or D // heads not in HEAD_SIZES:
        return False
    if (causal and L < S) or B > _MAX_GRID or heads > _MAX_GRID:
        return False
    if any((t.shape[1] - 1) * t.stride(1) + D >= _MAX_SLICE for t in (q, k, v) if t.stride(2) == 1):
        return False
    if key_add is not None and not (key_add.is_cuda and key_add.shape == (B, L)):
        return False
    return bias is None or _bias_ok(bias, B, heads, S, L)


def _in_place(t: torch.Tensor) -> torch.Tensor:
    """t as the kernel reads it: unit stride along the last dimension, 16-byte aligned rows (a packed
    projection's slices are); anything else is copied"""
    if t.stride(2) == 1 and t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0:
        return t
    return t.contiguous()


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None,
              key_add: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
              causal: bool = False) -> torch.Tensor:
    """softmax(scale * q k^T + key_add + bias + causal) v per head -> [B, S, D] in the input dtype. ``scale``
    None: 1 / sqrt(head size). ``key_add`` [B, L] is added to every query row and head; ``bias``
    [B|1, heads|1, S|1, L] broadcasts over its size-1 dimensions; both are additive (fp32). ``causal``: key l is
    visible to query s iff l <= s + (L - S)."""
    if not supported(q, k, v, heads, key_add, bias, causal):
        raise ValueError("attention: operands not supported (see supported())")
    B, S, D = q.shape
    L, d = k.shape[1], D // heads
    q, k, v = _in_place(q), _in_place(k), _in_place(v)
    strides = []
    for t in (q, k, v):
        strides += [t.stride(0), t.stride(1), d]
    if key_add is not None:
        key_add = key_add.to(torch.float32).contiguous()
    if bias is not None:
        bias = bias.to(torch.float32)
        if bias.stride(3) != 1 and L > 1:
            bias = bias.contiguous()
        strides += [0 if bias.shape[i] == 1 else bias.stride(i) for i in range(3)]
    else:
        strides += [0, 0, 0]
    out = torch.empty((B, S, D), device=q.device, dtype=q.dtype)
    sc = float(scale) if scale else 1.0 / math.sqrt(d)
    took = native.load("_nn").attention(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), [B, heads, S, L, d, int(bool(causal))], strides, sc,
        0 if key_add is None else key_add.data_ptr(), 0 if bias is None else bias.data_ptr(), _DT[q.dtype],
        torch.cuda.current_stream(q.device).cuda_stream)
    if not took:
        raise RuntimeError("attention: shape not supported by the kernel (check supported() first)")
    return out
