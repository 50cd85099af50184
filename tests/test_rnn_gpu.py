"""K24 fused persistent LSTM / GRU (csrc/nn/rnn_mfma.hip, ops.rnn) against a plain fp64 numpy recurrence on the
same fp32 inputs. The recurrence compounds rounding over T, so the bound is relative to the unfused fp32 time loop
(SML_RNN=0) run in the same process on the same inputs: max|new - ref| <= 4 max|old - ref| + 1e-6 (4: another
summation order and another exp; 1e-6: a floor for when the old path is exact to the last bit; outputs are bounded
by max(1, |h0|))."""
import functools

import numpy as np
import pytest
import torch

from synapseml_amd.onnx import InferenceSession, proto as P
from synapseml_amd.onnx.writer import GraphBuilder
from synapseml_amd.ops import rnn

pytestmark = pytest.mark.gpu
# (T, N, I, H, nd): H below a unit tile and N below a batch tile; exact tiles, one step; ragged second batch tile
# with H padded 40 -> 48; 9 unit tiles; 17 tiles on the 4-slot kernel (uneven over waves); 32 tiles on 8 waves,
# LDS above 64 KiB
SHAPES = [(6, 3, 4, 5, 2), (1, 16, 8, 16, 1), (9, 17, 3, 40, 2), (5, 33, 16, 136, 1), (3, 5, 4, 264, 1),
          (2, 3, 4, 500, 1)]
VARIANTS = {"LSTM": {"plain": {}, "peep_clip": {"clip": 1.5}, "input_forget": {"input_forget": 1}},
            "GRU": {"lbr0": {"linear_before_reset": 0}, "lbr1": {"linear_before_reset": 1}}}
CASES = [(c, s, v) for c in VARIANTS for s in SHAPES for v in VARIANTS[c]]
IDS = [f"{c}-{v}-{'x'.join(map(str, s))}" for c, s, v in CASES]


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _ref(cell, X, W, R, B, lens, h0, c0, Pp, reverse, at):
    """one direction, fp64, item by item: Y [T, N, H] (zeros past each length), final h and c"""
    (T, N, _), H, G = X.shape, R.shape[-1], 4 if cell == "LSTM" else 3
    X, W, R, B, Pp = (np.asarray(a, np.float64) for a in (X, W, R, B, Pp))
    clip = at.get("clip")
    cl = (lambda v: np.clip(v, -clip, clip)) if clip else (lambda v: v)
    Y, h, c = np.zeros((T, N, H)), np.array(h0, np.float64), np.array(c0, np.float64)
    Wb, Rb = B[:G * H], B[G * H:]
    for n in range(N):
        hn, cn = h[n], c[n]
        for t in (range(lens[n] - 1, -1, -1) if reverse else range(lens[n])):
            if cell == "LSTM":
                zi, zo, zf, zc = np.split(cl(X[t, n] @ W.T + hn @ R.T + Wb + Rb), 4)
                i = _sig(zi + Pp[:H] * cn)
                f = 1 - i if at.get("input_forget") else _sig(zf + Pp[2 * H:] * cn)
                cn = f * cn + i * np.tanh(zc)
                hn = _sig(zo + Pp[H:2 * H] * cn) * np.tanh(cn)
            else:
                (xz, xr, xh), (Rz, Rr, Rh), (bz, br, bh) = (np.split(a, 3) for a in (X[t, n] @ W.T + Wb, R, Rb))
                z, r = _sig(cl(xz + hn @ Rz.T + bz)), _sig(cl(xr + hn @ Rr.T + br))
                inner = r * (hn @ Rh.T + bh) if at["linear_before_reset"] else (r * hn) @ Rh.T + bh
                hn = (1 - z) * np.tanh(cl(xh + inner)) + z * hn
            Y[t, n] = hn
        h[n], c[n] = hn, cn
    return Y, h, c


def _inputs(cell, shape, variant, seed=0):
    """layout-0 numpy inputs; weights ~ 1 / sqrt(fan-in): pre-activations of standard deviation near 1"""
    (T, N, I, H, nd), G = shape, 4 if cell == "LSTM" else 3
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    lens = rng.integers(1, T + 1, N).astype(np.int32)
    lens[:3] = [T, 1, 0][:min(N, 3)]
    d = {"X": f32(rng.standard_normal((T, N, I))), "W": f32(rng.standard_normal((nd, G * H, I)) / np.sqrt(I)),
         "R": f32(rng.standard_normal((nd, G * H, H)) / np.sqrt(H)),
         "B": f32(rng.standard_normal((nd, 2 * G * H)) * 0.1), "lens": lens, "h0": f32(rng.standard_normal((nd, N, H)) * 0.5)}
    if cell == "LSTM":
        d["c0"] = f32(rng.standard_normal((nd, N, H)) * 0.5)
        if variant == "peep_clip":
            d["P"] = f32(rng.standard_normal((nd, 3 * H)) * 0.2)
    return d


def _reference(cell, d, at, reverse_d0=False):
    """fp64 outputs of every direction stacked like the operator's: Y [T, nd, N, H], Y_h, Y_c [nd, N, H]"""
    nd, H = d["W"].shape[0], d["R"].shape[-1]
    per = [_ref(cell, d["X"], d["W"][k], d["R"][k], d["B"][k], d["lens"], d["h0"][k], d.get("c0", d["h0"])[k],
                d["P"][k] if "P" in d else np.zeros(3 * H), k == 1 or reverse_d0, at) for k in range(nd)]
    return [np.stack([p[i] for p in per], 1 if i == 0 else 0) for i in range(3 if cell == "LSTM" else 2)]


def _operator(cell, d, at, layout=0):
    """the ONNX operator through a device session -> outputs in layout 0"""
    order = ["X", "W", "R", "B", "lens", "h0", "c0", "P"]
    sw = (lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))) if layout else (lambda a: a)
    feeds = {k: sw(d[k]) if k in ("X", "h0", "c0") else d[k] for k in order if k in d}
    b = GraphBuilder(cell)
    for k, a in feeds.items():
        b.input(k, P.ONNX_OF[a.dtype], list(a.shape))
    n_out = 3 if cell == "LSTM" else 2
    attrs = dict(at, hidden_size=d["R"].shape[-1], layout=layout,
                 direction="bidirectional" if d["W"].shape[0] == 2 else "forward")
    for o in b.add(cell, [k if k in feeds else "" for k in order[:8 if cell == "LSTM" else 6]], attrs, n_out=n_out):
        b.output(o, P.FLOAT32, None)
    sess = InferenceSession(b.to_bytes(), device="cuda", optimization_level="NO_OPT")
    outs = [np.asarray(o) for o in sess.run(None, feeds)]
    return [outs[0].transpose(1, 2, 0, 3)] + [o.swapaxes(0, 1) for o in outs[1:]] if layout else outs


@functools.lru_cache(maxsize=None)
def _kernel(cell, shape, variant):
    """the kernel's outputs on the case's inputs (device sequence_lens); supported() is asserted first"""
    d, at = _inputs(cell, shape, variant), VARIANTS[cell][variant]
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    direction = "bidirectional" if shape[4] == 2 else "forward"
    states = (t["h0"], t["c0"]) if cell == "LSTM" else (t["h0"],)
    assert rnn.supported(t["X"], t["W"], t["R"], 4 if cell == "LSTM" else 3, t["B"], t["lens"], states, t.get("P"),
                         direction, at.get("clip"))
    if cell == "LSTM":
        out = rnn.lstm(t["X"], t["W"], t["R"], t["B"], t["lens"], t["h0"], t["c0"], t.get("P"), direction,
                       at.get("clip"), bool(at.get("input_forget")))
    else:
        out = rnn.gru(t["X"], t["W"], t["R"], t["B"], t["lens"], t["h0"], direction, None,
                      bool(at["linear_before_reset"]))
    return d, [o.cpu().numpy() for o in out]


def _err(outs, ref):
    return max(float(np.abs(o.astype(np.float64) - r).max()) for o, r in zip(outs, ref))


@pytest.mark.parametrize("cell,shape,variant", CASES, ids=IDS)
def test_kernel_against_fp64(monkeypatch, cell, shape, variant):
    d, new = _kernel(cell, shape, variant)
    at = VARIANTS[cell][variant]
    ref = _reference(cell, d, at)
    monkeypatch.setenv("SML_RNN", "0")
    e_old, e_new = _err(_operator(cell, d, at), ref), _err(new, ref)
    print(f"rnn {cell} {variant} {shape}: new {e_new:.3e} old {e_old:.3e} ratio {e_new / max(e_old, 1e-30):.2f}")
    assert e_new <= 4 * e_old + 1e-6


@pytest.mark.parametrize("cell,shape,variant", CASES, ids=IDS)
def test_masking_is_exact(cell, shape, variant):
    d, new = _kernel(cell, shape, variant)
    Y, Yh, lens = new[0], new[1], d["lens"]
    for n, ln in enumerate(lens):
        assert not Y[ln:, :, n].any()
        for k in range(shape[4]):
            last = (d["h0"][k, n] if ln == 0 else Y[0 if k == 1 else ln - 1, k, n])
            np.testing.assert_array_equal(Yh[k, n], last)
            if ln == 0 and cell == "LSTM":
                np.testing.assert_array_equal(new[2][k, n], d["c0"][k, n])


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("cell,variant", [("LSTM", "peep_clip"), ("GRU", "lbr0")])
def test_operator_reaches_the_kernel(monkeypatch, cell, variant, layout):
    shape, at = (9, 17, 3, 40, 2), VARIANTS[cell][variant]
    d = _inputs(cell, shape, variant, seed=1)
    ref = _reference(cell, d, at)
    calls = []
    entry = "lstm" if cell == "LSTM" else "gru"
    real = getattr(rnn, entry)
    monkeypatch.setattr(rnn, entry, lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setenv("SML_RNN", "0")
    e_old = _err(_operator(cell, d, at, layout), ref)
    assert not calls
    monkeypatch.setenv("SML_RNN", "1")
    e_new = _err(_operator(cell, d, at, layout), ref)
    print(f"rnn operator {cell} layout {layout}: new {e_new:.3e} old {e_old:.3e} ratio {e_new / max(e_old, 1e-30):.2f}")
    assert len(calls) == 1 and e_new <= 4 * e_old + 1e-6


def test_supported_declines():
    X, W, R = (torch.zeros(s, device="cuda") for s in ((4, 2, 3), (1, 20, 3), (1, 20, 5)))
    assert rnn.supported(X, W, R, 4)
    big = (torch.zeros(1, 3 * 528, 3, device="cuda"), torch.zeros(1, 3 * 528, 528, device="cuda"))
    for args in [(X.cpu(), W.cpu(), R.cpu(), 4), (X.half(), W.half(), R.half(), 4), (X, *big, 3), (X[:0], W, R, 4),
                 (X, W, R, 3), (X, W, R, 4, None, None, (), None, "bidirectional")]:
        assert not rnn.supported(*args)
    with pytest.raises(ValueError):
        rnn.lstm(X.cpu(), W.cpu(), R.cpu())
