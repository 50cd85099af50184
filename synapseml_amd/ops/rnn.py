"""Python entry to the fused persistent LSTM / GRU (K24, csrc/nn/rnn_mfma.hip): the device path of the ONNX
``LSTM`` and ``GRU`` operators. Operands are fp32 torch CUDA tensors in the ONNX layout-0 shapes: X [T, N, I],
W [nd, gates * H, I], R [nd, gates * H, H], B [nd, 2 * gates * H], sequence_lens [N], initial states [nd, N, H],
P [nd, 3 * H]. The input projection stays one batched GEMM in front of the kernel (with the biases folded in);
R is repacked into the kernel's fragment order by index arithmetic; one launch on the current stream then runs
every step of every direction. Nothing here reads a tensor value, so a call never waits for the device."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as Fn

from . import native

# a block streams all of R through one CU at every step: measured 13 - 27x the time loop at H 128 - 256, 2 - 2.7x
# at H = 512, but 0.72x at H = 640 and 0.53x at H = 1024 (profiles/r10/rnn): larger H keeps the time loop
MAX_HIDDEN = 512
DIRECTIONS = {"forward": 0, "reverse": 1, "bidirectional": 2}  # -> the kernel's reverse bits


def supported(X: torch.Tensor, W: torch.Tensor, R: torch.Tensor, gates: int, B: Optional[torch.Tensor] = None,
              sequence_lens: Optional[torch.Tensor] = None, states: Tuple[Optional[torch.Tensor], ...] = (),
              P: Optional[torch.Tensor] = None, direction: str = "forward", clip: Optional[float] = None) -> bool:
    """Whether the kernel takes this problem: ``gates`` 4 (LSTM) or 3 (GRU), every operand on X's device, fp32
    (sequence_lens: any integer type), 1 <= H <= MAX_HIDDEN, one or two directions matching ``direction``.
    Declined (the caller keeps its own path): host tensors, other dtypes, H > MAX_HIDDEN, empty tensors,
    shapes that do not fit together, a clip that is not positive."""
    if not (X.is_cuda and X.dtype == torch.float32 and X.dim() == 3 and X.numel()):
        return False
    if gates not in (3, 4) or direction not in DIRECTIONS or W.dim() != 3 or R.dim() != 3:
        return False
    (T, N, I), nd, H = X.shape, W.shape[0], R.shape[2]
    if nd != (2 if direction == "bidirectional" else 1) or not 1 <= H <= MAX_HIDDEN:
        return False
    if W.shape != (nd, gates * H, I) or R.shape != (nd, gates * H, H):
        return False
    want = [(W, W.shape), (R, R.shape), (B, (nd, 2 * gates * H)), (P, (nd, 3 * H))]
    want += [(s, (nd, N, H)) for s in states]
    for t, shape in want:
        if t is not None and not (t.device == X.device and t.dtype == torch.float32 and t.shape == shape):
            return False
    if sequence_lens is not None and not (sequence_lens.device == X.device and sequence_lens.shape == (N,)
                                          and not sequence_lens.is_floating_point()):
        return False
    return clip is None or clip > 0


def _pad_units(t: torch.Tensor, gates: int, H: int, Hp: int) -> torch.Tensor:
    """[nd, gates * H, ...] -> [nd, gates * Hp, ...]: every gate's H rows followed by Hp - H zero rows"""
    if Hp == H:
        return t
    g = t.reshape(t.shape[0], gates, H, *t.shape[2:])
    g = Fn.pad(g, [0, 0] * (g.dim() - 3) + [0, Hp - H])
    return g.reshape(t.shape[0], gates * Hp, *t.shape[2:])


def _pack_r(R: torch.Tensor, gates: int, H: int, Hp: int) -> torch.Tensor:
    """R [nd, gates * H, H] -> [nd][unit tile][gate][k chunk][lane][4]; lane = 16 * (k % 16 // 4) + unit % 16"""
    nd, nt = R.shape[0], Hp // 16
    Rp = Fn.pad(_pad_units(R, gates, H, Hp), [0, Hp - H])            # [nd, gates * Hp, Hp]
    Rp = Rp.reshape(nd, gates, nt, 16, nt, 4, 4)                      # d, g, u, unit, kc, k / 4, k % 4
    return Rp.permute(0, 2, 1, 4, 5, 3, 6).contiguous()               # d, u, g, kc, k / 4, unit, k % 4


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """contiguous and 16-byte aligned (a slice of a larger tensor may be neither)"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _run(cell: int, X, W, R, bias, lens, h0, c0, peep, rbh, direction, clip, lbr, coupled):
    (T, N, I), nd, H = X.shape, W.shape[0], R.shape[2]
    gates = 4 if cell == 0 else 3
    Hp = (H + 15) // 16 * 16
    Wp = _pad_units(W, gates, H, Hp)
    bp = _pad_units(bias.unsqueeze(2), gates, H, Hp).transpose(1, 2)  # [nd, 1, gates * Hp]
    xw = torch.baddbmm(bp, X.reshape(1, T * N, I).expand(nd, -1, -1), Wp.transpose(1, 2))  # [nd, T N, gates Hp]
    rp = _pack_r(R, gates, H, Hp)
    if lens is not None:
        lens = lens.to(torch.int32).contiguous()
    h0, c0 = (None if s is None else s.contiguous() for s in (h0, c0))
    if peep is not None:
        peep = _aligned(_pad_units(peep.unsqueeze(2), 3, H, Hp))
    if rbh is not None:
        rbh = _aligned(Fn.pad(rbh, [0, Hp - H]))
    y = torch.empty((T, nd, N, H), device=X.device, dtype=torch.float32)
    yh = torch.empty((nd, N, H), device=X.device, dtype=torch.float32)
    yc = torch.empty_like(yh) if cell == 0 else None
    ptrs = [0 if t is None else t.data_ptr() for t in (xw, rp, h0, c0, peep, rbh, lens, y, yh, yc)]
    took = native.load("_nn").rnn(ptrs, [cell, T, N, H, nd, DIRECTIONS[direction], int(lbr), int(coupled)],
                                  float(clip or 0.0), torch.cuda.current_stream(X.device).cuda_stream)
    if not took:
        raise RuntimeError("rnn: shape not supported by the kernel (check supported() first)")
    return y, yh, yc


def lstm(X: torch.Tensor, W: torch.Tensor, R: torch.Tensor, B: Optional[torch.Tensor] = None,
         sequence_lens: Optional[torch.Tensor] = None, h0: Optional[torch.Tensor] = None,
         c0: Optional[torch.Tensor] = None, P: Optional[torch.Tensor] = None, direction: str = "forward",
         clip: Optional[float] = None, input_forget: bool = False):
    """ONNX LSTM (gates i, o, f, c; Sigmoid, Tanh, Tanh) -> Y [T, nd, N, H] (zeros past each length), Y_h and Y_c
    [nd, N, H] (the state after each item's last step; the initial state for a length of 0)."""
    if not supported(X, W, R, 4, B, sequence_lens, (h0, c0), P, direction, clip):
        raise ValueError("lstm: operands not supported (see supported())")
    H = R.shape[2]
    bias = W.new_zeros(W.shape[0], 4 * H) if B is None else B[:, :4 * H] + B[:, 4 * H:]
    return _run(0, X, W, R, bias, sequence_lens, h0, c0, P, None, direction, clip, 0, input_forget)


def gru(X: torch.Tensor, W: torch.Tensor, R: torch.Tensor, B: Optional[torch.Tensor] = None,
        sequence_lens: Optional[torch.Tensor] = None, h0: Optional[torch.Tensor] = None,
        direction: str = "forward", clip: Optional[float] = None, linear_before_reset: bool = False):
    """ONNX GRU (gates z, r, h; Sigmoid, Tanh) -> Y [T, nd, N, H] (zeros past each length) and Y_h [nd, N, H]."""
    if not supported(X, W, R, 3, B, sequence_lens, (h0,), None, direction, clip):
        raise ValueError("gru: operands not supported (see supported())")
    H = R.shape[2]
    rbh = None
    if B is None:
        bias = W.new_zeros(W.shape[0], 3 * H)
    elif linear_before_reset:  # Rbh sits inside r . (h Rh^T + Rbh): the kernel adds it
        bias = B[:, :3 * H] + Fn.pad(B[:, 3 * H:5 * H], [0, H])
        rbh = B[:, 5 * H:]
    else:
        bias = B[:, :3 * H] + B[:, 3 * H:]
    y, yh, _ = _run(1, X, W, R, bias, sequence_lens, h0, None, None, rbh, direction, clip, linear_before_reset, 0)
    return y, yh
