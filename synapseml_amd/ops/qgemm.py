"""Python entry to the int8 MFMA GEMM (K18, csrc/nn/qgemm_mfma.hip): ONNX ``MatMulInteger`` /
``QLinearMatMul`` / ``ConvInteger`` / ``QLinearConv``. Operands are torch CUDA tensors, uint8 or int8 in any
combination; strides are read from the tensors, launches go on the current stream. Zero points, scales and
bias stay on the device and are read by the kernel: nothing here reads a tensor value, so a launch never
waits for the device. The integer accumulation is exact and the requantisation is the executor's host
expression in fp64, so the results equal the host path bit for bit."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import native
from .conv import out_hw

_QDT = (torch.uint8, torch.int8)
_OUT = {torch.int32: 0, torch.uint8: 1, torch.int8: 2}
MAX_K = 32768  # 255 * 255 * K < 2^31: every accumulator fits in int32
_MAX_BATCH = 65535


def _zp_ok(zp: Optional[torch.Tensor], dtype: torch.dtype, n: int) -> bool:
    return zp is None or (zp.dtype == dtype and zp.dim() <= 1 and zp.numel() in (1, n))


def supported(a: torch.Tensor, b: torch.Tensor, a_zp: Optional[torch.Tensor] = None,
              b_zp: Optional[torch.Tensor] = None, group: Optional[int] = None) -> bool:
    """Whether the kernel takes this problem. ``group`` None: matmul of ``a`` [..., M, K] and ``b``
    [..., K, N]; an int: the 2-D convolution of ``a`` = x [B, C, H, W] with ``b`` = w [Cout, C / group, R, S].
    Declined (the caller keeps its own path): other dtypes, host tensors, 1-D operands, 1-D / 3-D
    convolutions, groups narrower than 16 outputs, zero points of rank > 1, K > 32768."""
    if not (a.is_cuda and b.is_cuda and a.dtype in _QDT and b.dtype in _QDT and a.numel() and b.numel()):
        return False
    if group is None:
        if a.dim() < 2 or b.dim() < 2 or a.shape[-1] != b.shape[-2] or a.shape[-1] > MAX_K:
            return False
        try:
            batch = torch.broadcast_shapes(a.shape[:-2], b.shape[:-2])
        except RuntimeError:
            return False
        if torch.Size(batch).numel() > _MAX_BATCH:
            return False
        return _zp_ok(a_zp, a.dtype, a.shape[-2]) and _zp_ok(b_zp, b.dtype, b.shape[-1])
    if a.dim() != 4 or b.dim() != 4 or group < 1 or a.shape[1] % group or b.shape[0] % group:
        return False
    cout, cg, r, s = b.shape
    if cg != a.shape[1] // group or (group > 1 and cout // group < 16) or group > _MAX_BATCH:
        return False
    return r * s * cg <= MAX_K and _zp_ok(a_zp, a.dtype, 1) and _zp_ok(b_zp, b.dtype, cout)


def _vec(t: Optional[torch.Tensor], dev, dtype: Optional[torch.dtype] = None) -> Optional[torch.Tensor]:
    if t is None:
        return None
    return t.to(dev, dtype if dtype is not None else t.dtype).reshape(-1).contiguous()


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _stride(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None or t.numel() == 1 else 1


class _Quant:
    """the operands of one launch that the kernel reads through pointers (kept alive until the call returns)"""

    def __init__(self, a, b, a_zp, b_zp, n, a_scale=None, b_scale=None, y_scale=None, y_zp=None, bias=None):
        dev = a.device
        for zp, t in ((a_zp, a), (b_zp, b)):
            if zp is not None and zp.dtype != t.dtype:
                raise ValueError(f"zero point {zp.dtype} of a {t.dtype} operand")
        self.a_zp, self.b_zp = _vec(a_zp, dev), _vec(b_zp, dev)
        self.out = torch.int32
        self.a_s = self.b_s = self.y_s = self.y_zp = self.bias = None
        if y_zp is not None:
            if y_zp.dtype not in _QDT or y_zp.numel() != 1:
                raise ValueError("y_zero_point: one uint8 / int8 value")
            self.out = y_zp.dtype
            self.a_s, self.b_s, self.y_s = (_vec(t, dev, torch.float32) for t in (a_scale, b_scale, y_scale))
            if self.a_s.numel() != 1 or self.y_s.numel() != 1 or self.b_s.numel() not in (1, n):
                raise ValueError("scales: a and y scalar, b scalar or per column")
            self.y_zp = _vec(y_zp, dev)
            self.bias = _vec(bias, dev, torch.int32)
            if self.bias is not None and self.bias.numel() != n:
                raise ValueError(f"bias: {n} int32 values")

    def flags(self, trans_b: int, a, b):
        return [trans_b, int(a.dtype == torch.int8), int(b.dtype == torch.int8), _OUT[self.out], _stride(self.a_zp),
                _stride(self.b_zp), _stride(self.b_s)]

    def ptrs(self):
        return [_ptr(t) for t in (self.a_zp, self.b_zp, self.a_s, self.b_s, self.y_s, self.y_zp, self.bias)]


def _launch(*args) -> None:
    if not native.load("_nn").qgemm(*args):
        raise RuntimeError("qgemm: shape not supported by the kernel (check supported() first)")


def _matmul(a: torch.Tensor, b: torch.Tensor, q_args) -> torch.Tensor:
    if not supported(a, b, q_args[0], q_args[1]):
        raise ValueError("qgemm: operands not supported (see supported())")
    M, K = a.shape[-2:]
    N = b.shape[-1]
    batch_shape = torch.broadcast_shapes(a.shape[:-2], b.shape[:-2])
    nb = torch.Size(batch_shape).numel()
    q = _Quant(a, b, *q_args[:2], N, *q_args[2:])
    A = a.expand(*batch_shape, M, K).reshape(nb, M, K)
    B = b.expand(*batch_shape, K, N).reshape(nb, K, N)
    if not (A.stride(2) == 1 and A.stride(1) >= K):
        A = A.contiguous()
    # b [K, N] row-major is read through the transposing stage; a transposed view of an [N, K] weight in place
    if B.stride(2) == 1 and B.stride(1) >= N:
        tb, ldb = 0, B.stride(1)
    elif B.stride(1) == 1 and B.stride(2) >= K:
        tb, ldb = 1, B.stride(2)
    else:
        B = B.contiguous()
        tb, ldb = 0, N
    y = torch.empty((nb, M, N), device=a.device, dtype=q.out)
    _launch(A.data_ptr(), B.data_ptr(), y.data_ptr(), M, N, K, nb, A.stride(1), ldb, N,
            A.stride(0) if nb > 1 else 0, B.stride(0) if nb > 1 else 0, M * N, q.flags(tb, a, b), q.ptrs(), 0,
            torch.cuda.current_stream(a.device).cuda_stream)
    return y.reshape(*batch_shape, M, N)


def matmul_integer(a: torch.Tensor, b: torch.Tensor, a_zp: Optional[torch.Tensor] = None,
                   b_zp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(a - a_zp) @ (b - b_zp) in int32, numpy batch broadcasting. ``a_zp``: scalar or per row [M]; ``b_zp``:
    scalar or per column [N]; each of its operand's dtype."""
    return _matmul(a, b, (a_zp, b_zp))


def qlinear_matmul(a, a_scale, a_zp, b, b_scale, b_zp, y_scale, y_zp) -> torch.Tensor:
    """ONNX QLinearMatMul: the integer product requantised to ``y_zp``'s dtype (round half to even,
    saturating). ``b_scale``: scalar or per column."""
    return _matmul(a, b, (a_zp, b_zp, a_scale, b_scale, y_scale, y_zp))


def _conv(x: torch.Tensor, w: torch.Tensor, q_args, strides, pads, dilations, group: int) -> torch.Tensor:
    if not supported(x, w, q_args[0], q_args[1], group=group):
        raise ValueError("qgemm: convolution not supported (see supported())")
    B, C, H, W = x.shape
    cout, cg, r, s = w.shape
    ng, K = cout // group, r * s * cg
    strides, dilations = tuple(strides or (1, 1)), tuple(dilations or (1, 1))
    pads = tuple(pads or (0, 0, 0, 0))
    oh, ow = out_hw(H, W, r, s, strides, pads, dilations)
    if oh <= 0 or ow <= 0:
        raise ValueError("qgemm: empty convolution output")
    q = _Quant(x, w, *q_args[:2], cout, *q_args[2:])
    x = x.contiguous(memory_format=torch.channels_last)
    wp = w.permute(0, 2, 3, 1).contiguous()  # [Cout][R][S][C / group]
    y = torch.empty((B, cout, oh, ow), device=x.device, dtype=q.out, memory_format=torch.channels_last)
    # one batch entry per group: its input channels at offset g * cg, its weights / outputs at g * ng
    _launch(x.data_ptr(), wp.data_ptr(), y.data_ptr(), B * oh * ow, ng, K, group, 0, K, cout, cg, ng * K, ng,
            q.flags(1, x, w), q.ptrs(), ng, torch.cuda.current_stream(x.device).cuda_stream,
            [H, W, C, r, s, strides[0], strides[1], pads[0], pads[1], dilations[0], dilations[1], oh, ow])
    return y


def conv_integer(x: torch.Tensor, w: torch.Tensor, x_zp: Optional[torch.Tensor] = None,
                 w_zp: Optional[torch.Tensor] = None, strides: Optional[Sequence[int]] = None,
                 pads: Optional[Sequence[int]] = None, dilations: Optional[Sequence[int]] = None,
                 group: int = 1) -> torch.Tensor:
    """ONNX ConvInteger on an NCHW ``x`` and ``w`` [Cout, C / group, R, S]: int32, channels_last memory with
    the NCHW shape. ``pads`` = (top, left, bottom, right); the padding holds ``x_zp`` (scalar). ``w_zp``:
    scalar or per output channel."""
    return _conv(x, w, (x_zp, w_zp), strides, pads, dilations, group)


def qlinear_conv(x, x_scale, x_zp, w, w_scale, w_zp, y_scale, y_zp, bias: Optional[torch.Tensor] = None,
                 strides: Optional[Sequence[int]] = None, pads: Optional[Sequence[int]] = None,
                 dilations: Optional[Sequence[int]] = None, group: int = 1) -> torch.Tensor:
    """ONNX QLinearConv: conv_integer (+ int32 ``bias``) requantised to ``y_zp``'s dtype. ``w_scale``: scalar
    or per output channel."""
    return _conv(x, w, (x_zp, w_zp, x_scale, w_scale, y_scale, y_zp, bias), strides, pads, dilations, group)
