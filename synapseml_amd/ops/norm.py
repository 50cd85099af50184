"""Python entry to the fused row-normalisation and bias-activation kernels (K25, csrc/nn/norm_rows.hip): the
LayerNormalization / RMSNormalization / Skip(Simplified)LayerNormalization / EmbedLayerNormalization and
Gelu / BiasGelu / FastGelu / QuickGelu operators of the ONNX executor. Operands are torch CUDA tensors; the
activation is fp16, bf16 or fp32 and is read in place through its row stride, gamma / beta / bias keep their own
float dtype. Launches go on the current stream. ``supported`` answers from shapes, dtypes, strides and devices
alone: nothing here reads a tensor value, so a launch never waits for the device and captures into a graph.

One deviation from torch: ``embed_layer_norm`` clamps every id to its table, where torch indexing raises on an
id out of range."""
from __future__ import annotations

from typing import Optional

import torch

from . import native

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
MAX_N = 8192                 # longest row the kernel holds in registers
WAVE_MAX_N = 1024            # up to here a wave owns a row; longer rows take a whole block
PLAIN_LN_MAX_N = 1024        # a LayerNorm with nothing fused into it: longer rows stay on the library kernel,
                             # which is as fast or faster there (tools/bench_norm.py: 0.82x at 4096 x 4096 fp16)
MODES = {"erf": 0, "tanh": 1, "quick": 2}
_MAX_ROWS = (1 << 31) - 1


def _as_rows(x: torch.Tensor, nd: int):
    """(rows, N, row stride) of x seen as rows over its last nd dimensions, or None when those are not one
    contiguous block or the leading dimensions do not collapse to a single stride"""
    shape, st, k = x.shape, x.stride(), x.dim() - nd
    N = 1
    for d in range(x.dim() - 1, k - 1, -1):
        if shape[d] != 1 and st[d] != N:
            return None
        N *= shape[d]
    rows, rs = 1, None
    for d in range(k - 1, -1, -1):
        if shape[d] == 1:
            continue
        if rs is None:
            rs = st[d]
        elif st[d] != rs * rows:
            return None
        rows *= shape[d]
    return rows, N, (N if rs is None else rs)


def _param_ok(p: Optional[torch.Tensor], N: int, dev: torch.device) -> bool:
    return p is None or (p.device == dev and p.dtype in _DT and p.numel() == N)


def _vector_form(N: int, es: int, *rows) -> bool:
    """whether the kernel's 16-byte form applies: N a whole number of vectors, every (tensor, row pitch in
    elements) 16-byte aligned. Reads addresses and strides, no values."""
    return N % (16 // es) == 0 and all(t is None or (t.data_ptr() % 16 == 0 and (rs * t.element_size()) % 16 == 0)
                                       for t, rs in rows)


def supported(x: torch.Tensor, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None, *,
              skip: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, axis: int = -1,
              fast_only: bool = False) -> bool:
    """Whether the kernels take x normalised (or activated) over its dimensions from ``axis`` on. Declined (the
    caller keeps its own path): host tensors, empty tensors, integer or fp64 activations, more than MAX_N
    elements per row, a non-unit inner stride, trailing dimensions that are not one contiguous block or leading
    ones that do not collapse to one row stride, gamma / beta / bias that are not float device tensors of the
    row's size, a skip whose shape is not x's or x's trailing dimensions, operands on another device than x.
    ``fast_only`` (the executor's routing) also declines what the kernels take but were not measured to win:
    rows longer than WAVE_MAX_N that need the element-wise form (odd N, unaligned rows or parameters)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in _DT and x.numel() and x.dim()):
        return False
    if not -x.dim() <= axis < x.dim():
        return False
    geo = _as_rows(x, x.dim() - axis % x.dim())
    if geo is None or geo[1] > MAX_N or geo[0] > _MAX_ROWS:
        return False
    N = geo[1]
    if not all(_param_ok(p, N, x.device) for p in (gamma, beta, bias)):
        return False
    sgeo = None
    if skip is not None:
        if not (skip.device == x.device and skip.dtype == x.dtype and 0 < skip.dim() <= x.dim()
                and tuple(skip.shape) == tuple(x.shape[x.dim() - skip.dim():])):
            return False
        sgeo = _as_rows(skip, skip.dim() - max(0, axis % x.dim() - (x.dim() - skip.dim())))
        if sgeo is None or sgeo[1] != N:
            return False
    if fast_only and N > WAVE_MAX_N:
        return _vector_form(N, x.element_size(), (x, geo[2]), (skip, sgeo[2] if sgeo else 0),
                            *((p, 0) for p in (gamma, beta, bias) if p is not None and p.is_contiguous()))
    return True


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _dt(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else _DT[t.dtype]


def _flat(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if p is None else p.contiguous()


def layer_norm(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float, *,
               skip: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, rms: bool = False,
               want_sum: bool = False, want_stats: bool = False, axis: int = -1):
    """y = (v - mean) * inv_std * gamma + beta over the dimensions from ``axis`` on, v = x (+ skip (+ bias)), in
    fp32 with two-pass statistics; ``rms``: y = v * rsqrt(mean(v^2) + eps) * gamma (no mean, beta must be None).
    ``skip`` has x's shape or its trailing dimensions (broadcast over the leading ones). Returns y in x's dtype,
    or (y, sum, mean, inv_std) when ``want_sum`` / ``want_stats``: sum is v rounded once to x's dtype, mean and
    inv_std are fp32 with the normalised dimensions kept as 1; what was not asked for (and the RMS mean) is
    None."""
    if bias is not None and skip is None:
        raise ValueError("layer_norm: bias needs skip")
    if rms and beta is not None:
        raise ValueError("layer_norm: the RMS form has no beta")
    if not supported(x, gamma, beta, skip=skip, bias=bias, axis=axis):
        raise ValueError("layer_norm: operands not supported (see supported())")
    ax = axis % x.dim()
    rows, N, x_rs = _as_rows(x, x.dim() - ax)
    skip_rows = skip_rs = 0
    if skip is not None:
        skip_rows, _, skip_rs = _as_rows(skip, skip.dim() - max(0, ax - (x.dim() - skip.dim())))
    gamma, beta, bias = _flat(gamma), _flat(beta), _flat(bias)
    y = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    total = torch.empty(x.shape, device=x.device, dtype=x.dtype) if want_sum else None
    stat_shape = tuple(x.shape[:ax]) + (1,) * (x.dim() - ax)
    mean = torch.empty(stat_shape, device=x.device, dtype=torch.float32) if want_stats and not rms else None
    inv = torch.empty(stat_shape, device=x.device, dtype=torch.float32) if want_stats else None
    with torch.cuda.device(x.device):  # the launch sizes its grid for the current device
        took = native.load("_nn").norm_rows(
            [x.data_ptr(), _ptr(skip), _ptr(bias), _ptr(gamma), _ptr(beta), y.data_ptr(), _ptr(total), _ptr(mean),
             _ptr(inv), 0, 0, 0, 0, 0, 0],
            [rows, N, x_rs, skip_rs, skip_rows, int(bool(rms)), 0, 1, 0, 0, 0, _DT[x.dtype], _dt(bias), _dt(gamma),
             _dt(beta)], float(eps), torch.cuda.current_stream(x.device).cuda_stream)
    if not took:
        raise RuntimeError("layer_norm: not taken by the kernel (check supported() first)")
    return (y, total, mean, inv) if want_sum or want_stats else y


def embed_supported(ids: torch.Tensor, seg_ids: Optional[torch.Tensor], word: torch.Tensor, pos: torch.Tensor,
                    seg: Optional[torch.Tensor], gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                    pos_ids: Optional[torch.Tensor] = None, fast_only: bool = False) -> bool:
    """Whether the gather form takes the problem: ids [B, S] int32 or int64 (seg_ids and pos_ids like them,
    pos_ids [B, S] or [1, S]), contiguous non-empty tables [rows, N] of one dtype out of fp16 / bf16 / fp32,
    N <= MAX_N, everything on the word table's device; without pos_ids the position table must have S rows.
    ``fast_only``: as in supported()."""
    if not (word.is_cuda and ids.device == word.device and ids.dim() == 2 and ids.numel() and ids.dtype in (torch.int32, torch.int64)):
        return False
    if not (word.is_cuda and word.dim() == 2 and word.dtype in _DT and word.numel() and word.is_contiguous()):
        return False
    N = word.shape[1]
    tables = [pos] + ([seg] if seg_ids is not None else [])
    if any(t is None or t.device != word.device or t.dim() != 2 or t.dtype != word.dtype or t.shape[1] != N
           or not t.shape[0] or not t.is_contiguous() for t in tables):
        return False
    if N > MAX_N or max(t.shape[0] for t in [word] + tables) > _MAX_ROWS:
        return False
    if seg_ids is not None and not (seg_ids.device == word.device and seg_ids.dtype == ids.dtype and seg_ids.shape == ids.shape):
        return False
    if pos_ids is None:
        if pos.shape[0] < ids.shape[1]:
            return False
    elif not (pos_ids.device == word.device and pos_ids.dtype == ids.dtype and pos_ids.dim() == 2
              and pos_ids.shape[1] == ids.shape[1] and pos_ids.shape[0] in (1, ids.shape[0])):
        return False
    if not (_param_ok(gamma, N, word.device) and _param_ok(beta, N, word.device)):
        return False
    if fast_only and N > WAVE_MAX_N:
        return _vector_form(N, word.element_size(), *((t, N) for t in [word] + tables),
                            *((p, 0) for p in (gamma, beta) if p is not None and p.is_contiguous()))
    return True


def embed_layer_norm(ids: torch.Tensor, seg_ids: Optional[torch.Tensor], word: torch.Tensor, pos: torch.Tensor,
                     seg: Optional[torch.Tensor], gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                     eps: float, pos_ids: Optional[torch.Tensor] = None, want_sum: bool = False):
    """LayerNorm of word[ids] + pos[pos_ids] (+ seg[seg_ids]) -> [B, S, N] in the tables' dtype; positions are
    0 .. S - 1 per batch entry without ``pos_ids``. ``want_sum``: returns (y, sum) with the embedding sum
    rounded once from fp32. Ids are clamped to their table (torch indexing raises instead)."""
    if not embed_supported(ids, seg_ids, word, pos, seg, gamma, beta, pos_ids):
        raise ValueError("embed_layer_norm: operands not supported (see embed_supported())")
    B, S = ids.shape
    N = word.shape[1]
    ids = ids.contiguous()
    if seg_ids is not None:
        seg_ids = seg_ids.contiguous()
    else:
        seg = None
    if pos_ids is not None:
        pos_ids = pos_ids.expand(B, S).contiguous()
    gamma, beta = _flat(gamma), _flat(beta)
    y = torch.empty((B, S, N), device=word.device, dtype=word.dtype)
    total = torch.empty_like(y) if want_sum else None
    with torch.cuda.device(word.device):
        took = native.load("_nn").norm_rows(
            [0, 0, 0, _ptr(gamma), _ptr(beta), y.data_ptr(), _ptr(total), 0, 0, ids.data_ptr(), _ptr(pos_ids),
             _ptr(seg_ids), word.data_ptr(), pos.data_ptr(), _ptr(seg)],
            [B * S, N, 0, 0, 0, 0, int(ids.dtype == torch.int64), S, word.shape[0], pos.shape[0],
             0 if seg is None else seg.shape[0], _DT[word.dtype], 0, _dt(gamma), _dt(beta)], float(eps),
            torch.cuda.current_stream(word.device).cuda_stream)
    if not took:
        raise RuntimeError("embed_layer_norm: not taken by the kernel (check embed_supported() first)")
    return (y, total) if want_sum else y


def bias_act(x: torch.Tensor, bias: Optional[torch.Tensor], mode: str, alpha: float = 1.702) -> torch.Tensor:
    """act(x + bias) in x's dtype, fp32 math; bias [N] over the last dimension or None. ``mode``: "erf"
    (0.5 v (1 + erf(v / sqrt 2))), "tanh" (0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3)))) or "quick"
    (v sigmoid(alpha v))."""
    if mode not in MODES:
        raise ValueError(f"bias_act: mode {mode!r} is not one of {sorted(MODES)}")
    if not supported(x, bias=bias):
        raise ValueError("bias_act: operands not supported (see supported())")
    rows, N, x_rs = _as_rows(x, 1)
    bias = _flat(bias)
    y = torch.empty(x.shape, device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):
        took = native.load("_nn").bias_act(x.data_ptr(), _ptr(bias), y.data_ptr(),
                                           [rows, N, x_rs, MODES[mode], _DT[x.dtype], _dt(bias)], float(alpha),
                                           torch.cuda.current_stream(x.device).cuda_stream)
    if not took:
        raise RuntimeError("bias_act: not taken by the kernel (check supported() first)")
    return y
