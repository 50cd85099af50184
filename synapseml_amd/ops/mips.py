"""Python entry to the fused MFMA top-k inner-product search (K23, csrc/nn/mips_topk.hip): the device path of
``KNN`` / ``ConditionalKNN``. Operands are torch CUDA fp32 tensors; queries and keys are read in place through
their row pitch when rows have unit stride and 16-byte alignment, launches go on the current stream. The
conditioner stays on the device (a label id per key, a bitset of eligible labels per query) and the split count
comes from the shapes alone: nothing here reads a tensor value, so a launch never waits for the device."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import native

MAX_K = 64
MAX_LABELS = 2048          # bits of a query's allow row the kernel keeps in LDS (kMipsMaxLabels)
_MAX_PITCH = 1 << 21       # floats: 32-bit byte offsets inside one key tile
_MAX_N = (1 << 31) - 256


def allow_words(n_labels: int) -> int:
    """uint32 words of one query's bitset over ``n_labels`` dense label ids"""
    return max(1, (n_labels + 31) // 32)


def supported(q: torch.Tensor, keys: torch.Tensor, k: int, key_label: Optional[torch.Tensor] = None,
              allow: Optional[torch.Tensor] = None) -> bool:
    """Whether the kernel takes this problem: q [M, D] and keys [N, D] fp32 on the device, non-empty,
    1 <= k <= 64; with a conditioner, ``key_label`` int32 [N] and ``allow`` [M, W] int32 / uint32 words on the
    device with 32 W <= MAX_LABELS. Declined (the caller keeps its own path): anything else."""
    if not (isinstance(q, torch.Tensor) and isinstance(keys, torch.Tensor) and q.is_cuda and keys.is_cuda):
        return False
    if q.dtype != torch.float32 or keys.dtype != torch.float32 or q.dim() != 2 or keys.dim() != 2:
        return False
    if q.shape[1] != keys.shape[1] or not (q.numel() and keys.numel()) or not 1 <= int(k) <= MAX_K:
        return False
    if keys.shape[0] > _MAX_N or q.shape[1] > _MAX_PITCH:
        return False
    if (key_label is None) != (allow is None):
        return False
    if key_label is not None:
        if not (key_label.is_cuda and key_label.dtype == torch.int32 and key_label.shape == (keys.shape[0],)):
            return False
        if not (allow.is_cuda and allow.dtype in (torch.int32, torch.uint32) and allow.dim() == 2
                and allow.shape[0] == q.shape[0] and 1 <= allow.shape[1] <= MAX_LABELS // 32):
            return False
    return True


def _rows(t: torch.Tensor) -> torch.Tensor:
    """t as the kernel reads it: unit stride along D, rows 16-byte aligned and readable up to D rounded up to
    4 floats; anything else is copied into zero-padded rows"""
    D = t.shape[1]
    if (D % 4 == 0 and t.stride(1) == 1 and t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0
            and D <= t.stride(0) <= _MAX_PITCH):
        return t
    if D % 4 == 0:
        return t.contiguous()
    out = torch.zeros((t.shape[0], (D + 3) // 4 * 4), device=t.device, dtype=t.dtype)
    out[:, :D] = t
    return out


def plan_splits(M: int, N: int, k: int, conditioned: bool = False) -> int:
    """key splits the kernel would take for these shapes on the current device"""
    return int(native.load("_nn").mips_split_plan(int(M), int(N), int(k), int(bool(conditioned))))


def topk(q: torch.Tensor, keys: torch.Tensor, k: int, key_label: Optional[torch.Tensor] = None,
         allow: Optional[torch.Tensor] = None, splits: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(vals fp32 [M, k], idx int32 [M, k]): per query the k largest inner products with the keys, descending,
    ties by the smaller key index; slots that cannot be filled hold -inf / -1. ``key_label`` / ``allow``: key n
    is eligible for query m iff bit ``key_label[n]`` of row ``allow[m]`` is set. ``splits``: blocks that share
    the keys of one query tile (None: from the shapes and the CU count). Scores must be finite."""
    if not supported(q, keys, k, key_label, allow):
        raise ValueError("mips.topk: operands not supported (see supported())")
    M, D = q.shape
    N, k = keys.shape[0], int(k)
    q, keys = _rows(q), _rows(keys)
    W = 0
    if key_label is not None:
        key_label, allow = key_label.contiguous(), allow.contiguous()
        W = allow.shape[1]
    mod = native.load("_nn")
    tiles = (N + 127) // 128
    s = plan_splits(M, N, k, key_label is not None) if splits is None else int(splits)
    s = max(1, min(s, tiles, 65535))
    vals = torch.empty((M, k), device=q.device, dtype=torch.float32)
    idx = torch.empty((M, k), device=q.device, dtype=torch.int32)
    ws = torch.empty((s, M, k), device=q.device, dtype=torch.int64) if s > 1 else None
    took = mod.mips_topk(q.data_ptr(), keys.data_ptr(), vals.data_ptr(), idx.data_ptr(), [M, N, D, k, W, s],
                         [q.stride(0), keys.stride(0)], 0 if key_label is None else key_label.data_ptr(),
                         0 if allow is None else allow.data_ptr(), 0 if ws is None else ws.data_ptr(),
                         torch.cuda.current_stream(q.device).cuda_stream)
    if not took:
        raise RuntimeError("mips.topk: shape not supported by the kernel (check supported() first)")
    return vals, idx
