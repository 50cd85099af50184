"""K25 fused row normalisation and bias-activation kernels (csrc/nn/norm_rows.hip, ops.norm) against fp64 numpy
formulas on the same inputs after rounding to the activation dtype.

Bound of the normalisation tests, derived and not tuned: |y - ref| <= u_out |ref| + E32. u_out is the unit
round-off of the output dtype (2^-24, 2^-11, 2^-8): one rounding of the result. E32 bounds the fp32 evaluation of
y = x_hat gamma + beta with x_hat = (v - mean) inv: a sum of N fp32 terms in any order is off by at most
(N - 1) u32 sum|t_i| (Higham, Accuracy and Stability, eq. 4.4), which bounds the relative error of the mean and
of the variance by N u32 each (the variance enters inv by half); the division by N, the subtraction, the square,
+ eps, the square root, the reciprocal and the three operations of the epilogue add one u32 each, 8 in all. So
E32 = (N + 8) u32 (max|gamma| max|x_hat| + max|beta|), u32 = 2^-24. The statistics outputs get the same term
relative to max|v| (mean) and to inv itself. The sum output is one rounding of the exact sum: u_out |sum|.

Cancellation: with rows 1000 + randn at N = 1024 a one-pass variance E[x^2] - mean^2 loses about 1e6 2^-24 = 0.06
of the unit variance. test_cancellation confirms with a numpy fp32 emulation of both formulas (same summation
order as the kernel: 16 sequential terms per lane, then a pairwise tree) that the two-pass form meets the bound
and the one-pass form misses it, before it checks the kernel.

bias_act: |y - ref| <= u_out |ref| + 2 e_t, where e_t is the largest error of torch's own fp32 formula
(Fn.gelu, the tanh formula, v sigmoid(alpha v)) against fp64 on the same inputs, measured in the test: two
correct fp32 implementations may round differently. The ROCm headers here state no ulp accuracy for erfcf / expf.
e_t is an absolute error set by |v| near 12, so test_act_negative_tail checks the tail relatively.

Operator tests: the kernel path (the torch bodies are patched to fail) is within twice the error of the
SML_NORM=0 path on the same inputs, and graph replays are bit-equal to the eager run."""
import gc
import math

import numpy as np
import pytest
import torch

from synapseml_amd.onnx import InferenceSession, ops as onnx_ops, ops_ext, proto as P
from synapseml_amd.onnx.writer import GraphBuilder
from synapseml_amd.ops import norm as NR

pytestmark = pytest.mark.gpu
U = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
U32 = 2.0 ** -24
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
F16_F32 = pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
RMS = pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
EPS = 1e-5


def _np(t):
    return None if t is None else t.detach().cpu().to(torch.float64).numpy()


def _dev(a, dtype):
    return torch.from_numpy(np.asarray(a)).to("cuda", dtype)


def _ref(v, gamma, beta, rms):
    """fp64 (y, x_hat, mean, inv) of rows v"""
    mean = 0.0 * v[..., :1] if rms else v.mean(-1, keepdims=True)
    inv = 1.0 / np.sqrt(((v - mean) ** 2).mean(-1, keepdims=True) + EPS)
    xh = (v - mean) * inv
    return xh * (1.0 if gamma is None else gamma) + (0.0 if beta is None else beta), xh, mean, inv


def _check(y, v, gamma, beta, rms, dtype):
    ref, xh, _, _ = _ref(v, gamma, beta, rms)
    e32 = (v.shape[-1] + 8) * U32 * (np.abs(gamma).max() * np.abs(xh).max() + (0.0 if beta is None else np.abs(beta).max()))
    over = float((np.abs(_np(y) - ref) - U[dtype] * np.abs(ref)).max())
    print(f"error beyond the output rounding {over:.3e} = {over / e32:.3f} E32 ({e32:.3e})")
    assert y.dtype == dtype and y.shape == v.shape and over <= e32


def _inputs(rows, N, dtype, seed, pdtype=None, rms=False):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, N, generator=g) * 2 + 0.5).to("cuda", dtype)
    gamma = (1 + 0.5 * torch.randn(N, generator=g)).to("cuda", pdtype or dtype)
    beta = None if rms else (0.5 * torch.randn(N, generator=g)).to("cuda", pdtype or dtype)
    return x, gamma, beta


@RMS
@DTYPES
@pytest.mark.parametrize("rows,N", [(1, 1), (3, 7), (5, 8), (4, 520), (9, 1024), (2, 1032), (3, 8192), (3, 1030)])
def test_layer_norm(rows, N, dtype, rms):
    x, gamma, beta = _inputs(rows, N, dtype, 1, rms=rms)
    assert NR.supported(x, gamma, beta)
    _check(NR.layer_norm(x, gamma, beta, EPS, rms=rms), _np(x), _np(gamma), _np(beta), rms, dtype)


@RMS
@pytest.mark.parametrize("form", ["row_stride", "fp32_params", "axis"])
def test_layer_norm_forms(form, rms):
    """a column slice of a wider tensor, fp32 gamma / beta on an fp16 activation, two trailing dimensions"""
    wide, gamma, beta = _inputs(6, 600, torch.float16, 2, torch.float32 if form == "fp32_params" else None, rms)
    x = wide[:, 40:560] if form == "row_stride" else wide[:, :520].contiguous()
    gamma, beta = gamma[:520], None if rms else beta[:520]
    assert form != "row_stride" or (x.stride(0) == 600 and not x.is_contiguous())
    if form == "axis":
        y = NR.layer_norm(x.reshape(6, 4, 130), gamma.reshape(4, 130), None if rms else beta.reshape(4, 130), EPS,
                          rms=rms, axis=1).reshape(6, 520)
    else:
        y = NR.layer_norm(x, gamma, beta, EPS, rms=rms)
    _check(y, _np(x), _np(gamma), _np(beta), rms, torch.float16)


def _f32_sum(t):
    """fp32 sum over the last axis in the kernel's order: 16 sequential terms per lane, then a pairwise tree"""
    s = t.reshape(-1, 4, 64, 4).transpose(0, 2, 1, 3).reshape(-1, 64, 16).cumsum(-1, dtype=np.float32)[..., -1]
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return s


def test_cancellation():
    g = torch.Generator().manual_seed(3)
    x = (1000 + torch.randn(8, 1024, generator=g)).cuda()
    gamma, beta = (1 + 0.5 * torch.randn(1024, generator=g)).cuda(), torch.randn(1024, generator=g).cuda()
    v, gn, bn = x.cpu().numpy(), gamma.cpu().numpy(), beta.cpu().numpy()
    n, eps = np.float32(1024), np.float32(EPS)
    mean = _f32_sum(v) / n
    two = (v - mean) / np.sqrt(_f32_sum((v - mean) ** 2) / n + eps) * gn + bn
    one = (v - mean) / np.sqrt(_f32_sum(v * v) / n - mean * mean + eps) * gn + bn
    assert two.dtype == np.float32 and one.dtype == np.float32
    _check(torch.from_numpy(two), _np(x), _np(gamma), _np(beta), False, torch.float32)
    with pytest.raises(AssertionError):
        _check(torch.from_numpy(one), _np(x), _np(gamma), _np(beta), False, torch.float32)
    _check(NR.layer_norm(x, gamma, beta, EPS), _np(x), _np(gamma), _np(beta), False, torch.float32)


@RMS
@F16_F32
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("bcast", [False, True], ids=["skip_full", "skip_bcast"])
@pytest.mark.parametrize("lead,N", [((2, 5), 72), ((2, 3), 1040)])
def test_skip_sum_stats(lead, N, bcast, with_bias, dtype, rms):
    g = torch.Generator().manual_seed(4)
    x, gamma, beta = _inputs(lead[0] * lead[1], N, dtype, 5, rms=rms)
    x = x.reshape(*lead, N)
    skip = torch.randn(*(lead[1:] if bcast else lead), N, generator=g).to("cuda", dtype)
    bias = torch.randn(N, generator=g).to("cuda", dtype) if with_bias else None
    assert NR.supported(x, gamma, beta, skip=skip, bias=bias)
    y, s, mean, inv = NR.layer_norm(x, gamma, beta, EPS, skip=skip, bias=bias, rms=rms, want_sum=True, want_stats=True)
    v = _np(x) + _np(skip) + (0.0 if bias is None else _np(bias))
    _, _, mean_ref, inv_ref = _ref(v, None, None, rms)
    _check(y, v, _np(gamma), _np(beta), rms, dtype)
    assert s.dtype == dtype and (np.abs(_np(s) - v) <= U[dtype] * np.abs(v)).all()
    assert (np.abs(_np(inv) - inv_ref) <= (N + 8) * U32 * inv_ref).all() and inv.shape == (*lead, 1)
    assert mean is None if rms else (np.abs(_np(mean) - mean_ref) <= (N + 8) * U32 * np.abs(v).max()).all()
    assert torch.equal(y, NR.layer_norm(x, gamma, beta, EPS, skip=skip, bias=bias, rms=rms))


@F16_F32
@pytest.mark.parametrize("with_pos_ids", [False, True], ids=["arange", "pos_ids"])
@pytest.mark.parametrize("with_seg", [False, True], ids=["noseg", "seg"])
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("N", [24, 1032])
def test_embed_layer_norm(N, idt, with_seg, with_pos_ids, dtype):
    g = torch.Generator().manual_seed(6)
    B, S = 2, 9
    word, pos, seg = (torch.randn(n, N, generator=g).to("cuda", dtype) for n in (11, 16, 2))
    gamma, beta = (1 + 0.5 * torch.randn(N, generator=g)).to("cuda", dtype), torch.randn(N, generator=g).to("cuda", dtype)
    ids = torch.randint(0, 11, (B, S), generator=g)
    ids[0, 0], ids[1, -1] = 0, 10
    seg_ids = (torch.arange(B * S).reshape(B, S) % 2) if with_seg else None
    pos_ids = torch.tensor([[15, 0, 3, 7, 7, 1, 14, 2, 9]]) if with_pos_ids else None
    dev = [None if t is None else t.to("cuda", idt) for t in (ids, seg_ids, pos_ids)]
    assert NR.embed_supported(dev[0], dev[1], word, pos, seg, gamma, beta, dev[2])
    y, s = NR.embed_layer_norm(dev[0], dev[1], word, pos, seg, gamma, beta, EPS, dev[2], want_sum=True)
    v = _np(word)[ids.numpy()] + _np(pos)[(pos_ids if with_pos_ids else torch.arange(S)).expand(B, S).numpy()]
    if with_seg:
        v = v + _np(seg)[seg_ids.numpy()]
    _check(y, v, _np(gamma), _np(beta), False, dtype)
    assert (np.abs(_np(s) - v) <= U[dtype] * np.abs(v)).all()


def _act_ref(v, mode):
    if mode == "erf":
        return 0.5 * v * (1.0 + np.vectorize(math.erf)(v / math.sqrt(2.0)))
    if mode == "tanh":
        return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
    return v / (1.0 + np.exp(-1.702 * v))


_TORCH_ACT = {"erf": torch.nn.functional.gelu, "tanh": ops_ext._gelu_tanh, "quick": lambda v: v * torch.sigmoid(1.702 * v)}


@DTYPES
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", [(3, 7), (5, 4096), (2, 3, 1000)])
@pytest.mark.parametrize("mode", ["erf", "tanh", "quick"])
def test_bias_act(mode, shape, with_bias, dtype):
    """measured on an MI355X: e_t between 7.1e-7 and 1.15e-6 over the cases (inputs up to |v| = 12); the kernel's
    error beyond the output rounding was at most 0.73 e_t"""
    g = torch.Generator().manual_seed(7)
    x = torch.rand(shape, generator=g) * 24 - 12
    x.view(-1)[0], x.view(-1)[-1] = -12.0, 12.0
    x = x.to("cuda", dtype)
    bias = (0.5 * torch.randn(shape[-1], generator=g)).to("cuda", dtype) if with_bias else None
    y = NR.bias_act(x, bias, mode)
    v32 = x.float() if bias is None else x.float() + bias.float()
    ref = _act_ref(_np(x) + (0.0 if bias is None else _np(bias)), mode)
    e_t = float(np.abs(_np(_TORCH_ACT[mode](v32)) - ref).max())
    over = float((np.abs(_np(y) - ref) - U[dtype] * np.abs(ref)).max())
    print(f"error beyond the output rounding {over:.3e}; torch fp32 formula error e_t {e_t:.3e}")
    assert y.dtype == dtype and y.shape == x.shape and over <= 2 * e_t


@pytest.mark.parametrize("mode", ["erf", "tanh", "quick"])
def test_act_negative_tail(mode):
    """fp32, v in [-6, -2], relative: the results fall to 1e-9 |v|, where test_bias_act's absolute bound says
    nothing and a 1 + erf(v / sqrt 2) or 1 + tanh(u) formulation has lost every digit. Bound 160 u32, reasoned:
    the result is v f(z) with f = erfc or 1 / (1 + exp), whose relative condition in z is at most 2 z^2 = v^2 <= 36
    (erfc) or |z| <= 25 (exp, z = 2 u); z carries at most 5 roundings (125 u32), the function itself at most
    OpenCL's bounds of 16 ulp (erfc) / 3 ulp (exp) = 32 u32, and three more operations follow."""
    x = torch.linspace(-6.0, -2.0, 4096, device="cuda").reshape(4, 1024)
    ref = _act_ref(_np(x), mode)
    rel = float((np.abs(_np(NR.bias_act(x, None, mode)) - ref) / np.abs(ref)).max())
    print(f"max relative error {rel:.3e} = {rel / U32:.1f} u32")
    assert rel <= 160 * U32


def _run_op(op_type, inputs, attrs, n_out, use_graph=False, runs=1):
    b = GraphBuilder(op_type)
    for name, arr in inputs:
        if name:
            b.input(name, P.ONNX_OF[arr.dtype], list(arr.shape))
    outs = b.add(op_type, [n for n, _ in inputs], attrs, out="y", n_out=n_out,
                 domain="" if op_type == "LayerNormalization" else "com.microsoft")
    for o in [outs] if n_out == 1 else outs:
        b.output(o, P.FLOAT32, None)
    sess = InferenceSession(b.to_bytes(), device="cuda", precision="fp16", optimization_level="NO_OPT",
                            use_graph=use_graph)
    res = [[np.asarray(o, np.float64) for o in sess.run(None, {n: a for n, a in inputs if n})] for _ in range(runs)]
    del sess  # a captured graph and its memory pool go here, with the device idle, not at a later collection
    gc.collect()
    torch.cuda.synchronize()
    return res


def _f16(a):
    return a.astype(np.float16).astype(np.float64)


def _op_case(name):
    """(op type, inputs, attributes, fp64 reference outputs, (module, torch body) to patch); hidden size 72"""
    rng = np.random.default_rng(8)
    B, S, N = 2, 5, 72
    x, skip = (rng.standard_normal((B, S, N)).astype(np.float32) * 2 for _ in range(2))
    gamma, beta, bias = (1 + 0.5 * rng.standard_normal(N)).astype(np.float32), *rng.standard_normal((2, N)).astype(np.float32)
    if name == "SkipLayerNormalization":
        v = _f16(x) + _f16(skip) + _f16(bias)
        y, _, mean, inv = _ref(v, _f16(gamma), _f16(beta), False)
        return (name, [("x", x), ("s", skip), ("g", gamma), ("b", beta), ("bias", bias)], {"epsilon": EPS},
                [y, mean, inv, v], (ops_ext, "_skip_ln_torch"))
    if name == "LayerNormalization":
        return (name, [("x", x), ("g", gamma), ("b", beta)], {"epsilon": EPS, "axis": -1},
                [_ref(_f16(x), _f16(gamma), _f16(beta), False)[0]], (onnx_ops, "_layer_norm_torch"))
    if name == "SimplifiedLayerNormalization":
        return (name, [("x", x), ("g", gamma)], {"epsilon": EPS, "axis": -1},
                [_ref(_f16(x), _f16(gamma), None, True)[0]], (ops_ext, "_rms"))
    if name == "EmbedLayerNormalization":
        word, pos, seg = (rng.standard_normal((n, N)).astype(np.float32) for n in (11, S, 2))
        ids, seg_ids = rng.integers(0, 11, (B, S)).astype(np.int32), rng.integers(0, 2, (B, S)).astype(np.int32)
        v = _f16(word)[ids] + _f16(pos)[None] + _f16(seg)[seg_ids]
        return (name, [("ids", ids), ("sid", seg_ids), ("w", word), ("p", pos), ("s", seg), ("g", gamma), ("b", beta)],
                {"epsilon": EPS}, [_ref(v, _f16(gamma), _f16(beta), False)[0], np.full(B, S, np.float64), v],
                (ops_ext, "_embed_ln_torch"))
    if name == "BiasGelu":
        return name, [("x", x), ("b", bias)], {}, [_act_ref(_f16(x) + _f16(bias), "erf")], (ops_ext, "_bias_gelu_torch")
    return name, [("x", x), ("b", bias)], {}, [_act_ref(_f16(x) + _f16(bias), "tanh")], (ops_ext, "_fast_gelu_torch")


@pytest.mark.parametrize("name", ["SkipLayerNormalization", "LayerNormalization", "SimplifiedLayerNormalization",
                                  "EmbedLayerNormalization", "BiasGelu", "FastGelu"])
def test_operator(monkeypatch, name):
    op_type, inputs, attrs, refs, (module, body) = _op_case(name)
    monkeypatch.setenv("SML_NORM", "0")
    parent = _run_op(op_type, inputs, attrs, len(refs))[0]
    monkeypatch.setenv("SML_NORM", "1")
    monkeypatch.setattr(module, body, lambda *a, **k: pytest.fail(f"fell back to {body}()"))
    eager = _run_op(op_type, inputs, attrs, len(refs))[0]
    for i, ref in enumerate(refs):
        err, perr = (float(np.abs(o[i].reshape(ref.shape) - ref).max()) for o in (eager, parent))
        print(f"{op_type} output {i}: kernel path max err {err:.3e}, torch path {perr:.3e}")
        assert err <= 2 * perr
    for replay in _run_op(op_type, inputs, attrs, len(refs), use_graph=True, runs=3):
        for got, want in zip(replay, eager):
            np.testing.assert_array_equal(got, want)


def test_supported():
    x = torch.zeros(4, 64, device="cuda", dtype=torch.float16)
    wide = torch.zeros(4, 8200, device="cuda", dtype=torch.float16)
    assert NR.supported(x) and NR.supported(x, x[0], x[0], skip=x, bias=x[0]) and NR.supported(wide[:, :8192])
    for bad in (x.cpu(), wide, wide[:, ::2], x.int(), x[:0]):
        assert not NR.supported(bad)
        for call in (lambda: NR.layer_norm(bad, None, None, EPS), lambda: NR.bias_act(bad, None, "erf")):
            with pytest.raises(ValueError):
                call()
    ids = torch.zeros(2, 3, device="cuda", dtype=torch.int64)
    assert NR.embed_supported(ids, None, x, x, None, None, None)
    with pytest.raises(ValueError):
        NR.embed_layer_norm(ids, None, x.cpu(), x, None, None, None, EPS)
