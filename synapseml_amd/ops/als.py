"""Python entry to the fused ALS half-sweep kernel (K27, csrc/nn/als_mfma.hip). ``prepare`` turns the ratings
into what the kernel walks, once per fit, with torch sorts on the device: the CSR of both orientations, and for each
the task table (rows longest first, rows longer than ``L`` cut into segments with workspace slots) and the table
of cut rows. ``half_sweep`` solves one side from the other on the current stream, in place, with workspace from
torch's allocator; ``supported`` answers from shapes, dtypes, devices and the host-side ratings alone."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import native

MAX_RANK = 64     # kAlsMaxRank
L = 2048          # nonzeros of a segment; a longer row is cut and summed by the reduce kernel


def padded_rank(k: int) -> int:
    return (k + 15) // 16 * 16


@dataclass
class Side:
    """one orientation; the tensors live on the device prepare() ran on"""
    n: int                   # rows of this side
    n_other: int             # rows of the side its indices name
    indices: torch.Tensor    # int32 [nnz]
    val: torch.Tensor        # fp64 [nnz]
    tasks: torch.Tensor      # int64 [rows + extra segments, 4]: row, first nonzero, length, slot; longest first,
                             # so the empty rows are the tail
    red: torch.Tensor        # int64 [cut rows, 4]: row, first slot, slots, nonzeros
    nonempty: int            # tasks of length > 0
    slots: int


@dataclass
class Prepared:
    sides: tuple             # (users x items, items x users)
    _dev: dict = field(default_factory=dict, repr=False)

    def on(self, dev: torch.device) -> tuple:
        """both sides' tensors on dev, moved once"""
        d = self._dev.get(dev)
        if d is None:
            d = tuple({n: getattr(s, n).to(dev) for n in ("indices", "val", "tasks", "red")} for s in self.sides)
            self._dev[dev] = d
        return d


def _side(rows, cols, val, n, n_other) -> Side:
    """CSR and tables of one orientation; (rows, cols) are unique and sorted by (row, col)"""
    dev = rows.device
    lens = torch.bincount(rows, minlength=n)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(lens, 0)
    nseg = torch.div(lens + L - 1, L, rounding_mode="floor").clamp(min=1)
    first = torch.cumsum(nseg, 0) - nseg
    row = torch.repeat_interleave(torch.arange(n, device=dev), nseg)
    seg = torch.arange(len(row), device=dev) - first[row]
    length = (lens[row] - seg * L).clamp(max=L)
    cut = nseg[row] > 1
    slot = torch.where(cut, torch.cumsum(cut, 0) - 1, -1)
    tasks = torch.stack([row, indptr[row] + seg * L, length, slot], 1)
    tasks = tasks[torch.sort(-length, stable=True).indices].contiguous()
    cut_rows = torch.nonzero(nseg > 1)[:, 0]
    slot0 = torch.cumsum(nseg[cut_rows], 0) - nseg[cut_rows]
    red = torch.stack([cut_rows, slot0, nseg[cut_rows], lens[cut_rows]], 1).contiguous()
    return Side(n=n, n_other=n_other, indices=cols.to(torch.int32), val=val.contiguous(), tasks=tasks, red=red,
                nonempty=int((length > 0).sum()), slots=int(cut.sum()))


def prepare(u, i, r, nU: int, nI: int) -> Prepared:
    """The kernel's view of the ratings r[j] of (u[j], i[j]) in an nU x nI problem. Of duplicate (u, i) pairs
    the last one counts, as in a dense scatter on the host. The sorts and the table builds run in torch, on the
    GPU where there is one."""
    u, i, r = np.asarray(u, np.int64), np.asarray(i, np.int64), np.asarray(r, np.float64)
    if not (len(u) == len(i) == len(r)) or not 0 < nU < 1 << 31 or not 0 < nI < 1 << 31:
        raise ValueError("als.prepare: u, i, r of one length and 0 < nU, nI < 2^31")
    if len(u) and (u.min() < 0 or i.min() < 0 or u.max() >= nU or i.max() >= nI):
        raise ValueError("als.prepare: an id is outside [0, nU) x [0, nI)")
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    u, i, r = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (u, i, r))
    key, by_key = torch.sort(u * nI + i, stable=True)
    last = torch.ones(len(key), dtype=torch.bool, device=dev)
    last[:-1] = key[1:] != key[:-1]
    keep = by_key[last]                                   # unique pairs, sorted by (u, i)
    u, i, r = u[keep], i[keep], r[keep]
    by_item = torch.sort(i * nU + u).indices              # sorted by (i, u)
    return Prepared((_side(u, i, r, nU, nI), _side(i[by_item], u[by_item], r[by_item], nI, nU)))


def supported(dev, rank: int, lam: float, u, i, r, implicit: bool) -> bool:
    """Whether the kernel takes this fit. Declined (the caller keeps its dense body): a host device, rank above
    MAX_RANK, a regularisation that is not positive, a negative id, and for implicit feedback a negative rating
    (the system can then be indefinite, and Cholesky is the wrong solver)."""
    u, i, r = np.asarray(u), np.asarray(i), np.asarray(r)
    return (torch.device(dev).type == "cuda" and 1 <= rank <= MAX_RANK and np.isfinite(lam) and lam > 0
            and len(u) > 0 and u.min() >= 0 and i.min() >= 0 and bool(np.isfinite(r).all())
            and not (implicit and r.min() < 0))


def factors(init: torch.Tensor, dev) -> torch.Tensor:
    """init [n, k] as the kernel's factor matrix on dev: an [n, k] view of zeroed fp64 [n, padded_rank(k)] storage,
    so every factor row starts on a 128-byte boundary"""
    n, k = init.shape
    out = torch.zeros(n, padded_rank(k), device=dev, dtype=torch.float64)[:, :k]
    out.copy_(init)
    return out


def half_sweep(prep: Prepared, side: int, X: torch.Tensor, Y: torch.Tensor, lam: float, alpha: float,
               implicit: bool, nonnegative: bool) -> None:
    """Solve X (side 0: the users' factors, side 1: the items') in place from the other side's Y; both as made by
    ``factors``. An explicit row without ratings keeps its value; an implicit one becomes zero."""
    s = prep.sides[side]
    k = X.shape[1] if isinstance(X, torch.Tensor) and X.dim() == 2 else 0
    kp = padded_rank(k)
    for t, n in ((X, s.n), (Y, s.n_other)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.shape == (n, k)
                and t.stride() == (kp, 1) and t.data_ptr() % 128 == 0 and t.device == X.device):
            raise ValueError(f"als.half_sweep: factors must be fp64 [{n}, {k}] views of pitch {kp} on one GPU "
                             "(see factors())")
    dev = X.device
    d = prep.on(dev)[side]
    ntasks = len(s.tasks) if implicit else s.nonempty
    slots = max(s.slots, (s.n_other + L - 1) // L if implicit else 0)
    per = kp * kp + kp
    with torch.cuda.device(dev):  # the launch sizes its grid for the current device
        ws = torch.empty(slots * per, device=dev, dtype=torch.float64) if slots else None
        yty = torch.empty(kp * kp, device=dev, dtype=torch.float64) if implicit else None

        def ptr(t):
            return 0 if t is None or t.numel() == 0 else t.data_ptr()

        took = native.load("_nn").als_sweep(
            [d["indices"].data_ptr(), d["val"].data_ptr(), d["tasks"].data_ptr(), ptr(d["red"]), Y.data_ptr(),
             X.data_ptr(), ptr(yty), ptr(ws)],
            [s.n, s.n_other, k, kp, ntasks, len(s.red), s.slots, slots * per, L, int(implicit), int(nonnegative)],
            [float(lam), float(alpha)], torch.cuda.current_stream(dev).cuda_stream)
    if not took:
        raise RuntimeError("als.half_sweep: not taken by the kernel (check supported() first)")
