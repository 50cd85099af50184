"""The ONNX executor's pointwise, pooling, softmax and direct-conv kernels (csrc/nn/nn_ops.hip,
csrc/nn/conv_direct.hip) and the float conv routes, against fp64 references at the shapes where such
kernels go wrong: scalar tails, NCHW / NHWC channel indexing, null pointers, in-place, partly filled
blocks, clamped pool windows, +-inf / NaN, odd conv geometry (dilation, asymmetric pads, rectangular
windows, unequal strides), and the dispatch guards in front of the kernels.

The pointwise checker's bound is derived, not measured: one rounding into the storage type plus the
fp32 arithmetic of a multiply and two adds. The CPU tests at the top prove that an fp32 emulation of each
kernel's arithmetic order passes it on the whole case table and that a set of subtly wrong kernels fails it."""
import itertools
import math
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_PREC = {torch.float32: (24, -126), torch.float16: (11, -14), torch.bfloat16: (8, -126)}  # (p, emin)
_U32 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------- checker
def spacing(ref: torch.Tensor, dtype) -> torch.Tensor:
    """Gap between neighbouring ``dtype`` values at |ref| (fp64): 2^(floor(log2|ref|) - p + 1), floored at
    the subnormal spacing 2^(emin - p + 1)."""
    p, emin = _PREC[dtype]
    _, e = torch.frexp(ref.double().abs())  # |ref| = m * 2^e, m in [0.5, 1): floor(log2|ref|) = e - 1
    fl = torch.where(ref == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), fl - p + 1)


def bound(ref, mag, dtype, extra=0.0):
    """|y - ref| <= 0.5 * spacing_T(ref) + 8 * 2^-24 * mag (+ extra)."""
    return 0.5 * spacing(ref, dtype) + 8 * _U32 * mag.double() + extra


def violations(y, ref, mag, dtype, extra=0.0):
    """Number of elements of ``y`` (storage type ``dtype``) outside the bound around the fp64 ``ref``, and
    the largest error."""
    err = (y.double().cpu() - ref.double()).abs()
    bad = ~(err <= bound(ref.double(), mag, dtype, extra))  # NaN counts as a violation
    return int(bad.sum()), float(err.max()) if err.numel() else 0.0


def check(y, ref, mag, dtype, extra=0.0, what=""):
    nbad, worst = violations(y, ref, mag, dtype, extra)
    assert nbad == 0, f"{what}: {nbad} of {ref.numel()} elements out of bound, largest error {worst:.3e}"


def test_spacing_matches_the_number_formats():
    for dt in _DTYPES:
        p, emin = _PREC[dt]
        v = torch.tensor([1.0, 1.5, 2.0, 3.5, 0.75, 1000.0, -5.0], dtype=torch.float64)
        got = spacing(v, dt)
        if dt == torch.float32:
            a = v.abs().float()
            assert torch.equal(got, (torch.nextafter(a, torch.full_like(a, math.inf)).double() - a.double()))
        assert got[0].item() == 2.0 ** (1 - p) and got[2].item() == 2.0 ** (2 - p) and got[4].item() == 2.0 ** (-p)
        assert spacing(torch.zeros(1, dtype=torch.float64), dt).item() == 2.0 ** (emin - p + 1)
        assert spacing(torch.tensor([2.0 ** (emin - 5)], dtype=torch.float64), dt).item() == 2.0 ** (emin - p + 1)
        assert torch.finfo(dt).eps == 2.0 ** (1 - p)


# ---------------------------------------------------------------------------------------------- pointwise cases
# (layout, logical shape): NHWC tensors are 4-D channels-last; NCHW ones are dense in their own order
_SHAPES = [
    (1, (2, 64, 7, 7)),     # vector path, n / 8 = 784: the fourth block is partly filled
    (1, (1, 8, 1, 1)),
    (1, (3, 12, 5, 3)),     # C % 8 != 0: all scalar
    (0, (2, 5, 4, 8)),      # HW % 8 == 0: vector path, one channel per vector
    (0, (2, 5, 3, 3)),      # HW % 8 != 0
    (0, (37, 10)),          # HW = 1
    (0, (2, 6, 16)),
    (0, (1, 4, 2, 3, 4)),
    (0, (1, 3, 1, 11)),     # n % 8 != 0: a tail inside a thread
]
_PTRS = [(1, 1, 1), (0, 1, 1), (0, 1, 0), (0, 0, 0)]  # (scale, shift, res) present
_ACTS = [(0, 0.0), (1, 0.0), (2, 0.1), (3, 0.0), (4, 6.0)]
_SIGMOID_EXTRA = 2e-6


def _shape_id(s):
    return ("nhwc" if s[0] else "nchw") + "x".join(map(str, s[1]))


def _chw(shape):
    return shape[1], int(np.prod(shape[2:])) if len(shape) > 2 else 1


def _bshape(shape):
    return [1, -1] + [1] * (len(shape) - 2)


def make_case(nhwc, shape, dtype, ptrs, act, alpha, seed):
    """Seeded inputs (CPU, logical layout). |pre-activation| <= 19 by construction (the sigmoid bound asks for
    <= 20); the first elements in memory are planted at about -3 and +9 before the activation so every case,
    however small, has inputs on both sides of 0 and above alpha = 6."""
    g = torch.Generator().manual_seed(seed)
    C, _ = _chw(shape)
    x = (4 * torch.randn(shape, generator=g)).clamp(-8, 8)
    scale = (torch.rand(C, generator=g) + 0.5) if ptrs[0] else None
    shift = torch.randn(C, generator=g).clamp(-3, 3) if ptrs[1] else None
    res = (2 * torch.randn(shape, generator=g)).clamp(-4, 4).to(dtype) if ptrs[2] else None
    bs = _bshape(shape)
    for i, target in ((0, -3.0), (1, 9.0)):
        # element i in memory order: (n, hw, c) for NHWC, the logical order otherwise
        idx = (0, i % C, (i // C) // shape[3], (i // C) % shape[3]) if nhwc else tuple(int(j) for j in np.unravel_index(i, shape))
        c = idx[1]
        t = target - (float(shift[c]) if shift is not None else 0.0) - (float(res[idx]) if res is not None else 0.0)
        x[idx] = t / (float(scale[c]) if scale is not None else 1.0)
    return types.SimpleNamespace(nhwc=nhwc, shape=tuple(shape), dtype=dtype, x=x.to(dtype), scale=scale, shift=shift,
                                 res=res, act=act, alpha=alpha, bs=bs)


def _act64(v, act, alpha):
    if act == 1:
        return v.clamp(min=0)
    if act == 2:
        return torch.where(v > 0, v, alpha * v)
    if act == 3:
        return torch.sigmoid(v)
    if act == 4:
        return v.clamp(0, alpha)
    return v


def affine_ref(c):
    """fp64 reference and the per-element magnitude (sum of |terms|)."""
    v = c.x.double()
    if c.scale is not None:
        v = v * c.scale.double().reshape(c.bs)
    mag = v.abs()
    if c.shift is not None:
        v = v + c.shift.double().reshape(c.bs)
        mag = mag + c.shift.double().abs().reshape(c.bs)
    if c.res is not None:
        v = v + c.res.double()
        mag = mag + c.res.double().abs()
    assert float(v.abs().max()) <= 20.0
    return _act64(v, c.act, c.alpha), mag


def _act32(v, act, alpha):
    if act == 1:
        return torch.clamp(v, min=0)
    if act == 2:
        return torch.where(v > 0, v, torch.tensor(alpha, dtype=torch.float32) * v)
    if act == 3:
        return 1.0 / (1.0 + torch.exp(-v))
    if act == 4:
        return torch.clamp(v, 0, alpha)
    return v


def _chan_vec(vec, c, mutation):
    """Per-channel vector broadcast to the tensor; the ``chan_mod`` mutation indexes channels as i % C over
    the memory order whatever the layout (right for NHWC, wrong for NCHW)."""
    if mutation == "chan_mod" and not c.nhwc:
        C, _ = _chw(c.shape)
        return vec[torch.arange(c.x.numel()) % C].reshape(c.shape)
    return vec.reshape(c.bs)


def affine_emulate(c, mutation=None):
    """The kernel's arithmetic order in fp32: multiply, add shift, add residual, activation, one rounding."""
    v = c.x.float()
    if c.scale is not None:
        v = v * _chan_vec(c.scale, c, mutation)
    if c.shift is not None and mutation != "no_shift":
        v = v + _chan_vec(c.shift, c, mutation)
    if mutation == "relu_before_res" and c.act == 1:
        v = torch.clamp(v, min=0)
        return (v + c.res.float()).to(c.dtype) if c.res is not None else v.to(c.dtype)
    if c.res is not None:
        v = v + c.res.float()
    alpha = c.alpha
    if mutation == "no_alpha":
        alpha = 0.0 if c.act == 2 else math.inf
    return _act32(v, c.act, alpha).to(c.dtype)


def _applies(mutation, c):
    """Whether the mutation changes the arithmetic of this case at all."""
    C, HW = _chw(c.shape)
    if mutation == "chan_mod":
        return not c.nhwc and HW > 1 and C > 1 and (c.scale is not None or c.shift is not None)
    if mutation == "no_shift":
        return c.shift is not None
    if mutation == "relu_before_res":
        return c.act == 1 and c.res is not None
    if mutation == "no_alpha":
        return c.act in (2, 4)
    raise AssertionError(mutation)


def affine_cases(shapes=_SHAPES):
    for si, (nhwc, shape) in enumerate(shapes):
        for dtype, ptrs, (act, alpha) in itertools.product(_DTYPES, _PTRS, _ACTS):
            seed = 1000 * si + 100 * _DT[dtype] + 10 * _PTRS.index(ptrs) + act
            yield make_case(nhwc, shape, dtype, ptrs, act, alpha, seed)


def add_case(nhwc, shape, dtype, act, seed):
    g = torch.Generator().manual_seed(seed)
    C, _ = _chw(shape)
    a = (3 * torch.randn(shape, generator=g)).to(dtype)
    b = (3 * torch.randn(shape, generator=g)).to(dtype)
    return types.SimpleNamespace(nhwc=nhwc, shape=tuple(shape), dtype=dtype, a=a, b=b, x=a, act=act,
                                 scale=torch.rand(C, generator=g) + 0.5, shift=torch.randn(C, generator=g),
                                 bs=_bshape(shape))


def add_cases(shapes=_SHAPES):
    for si, (nhwc, shape) in enumerate(shapes):
        for dtype, act in itertools.product(_DTYPES, (0, 1)):
            yield add_case(nhwc, shape, dtype, act, 5000 + 100 * si + 10 * _DT[dtype] + act)


def add_ref(c):
    s = (c.a.float() + c.b.float()).to(c.dtype)  # the kernel's first output, exactly
    t = s.double() * c.scale.double().reshape(c.bs)
    ref = t + c.shift.double().reshape(c.bs)
    return s, _act64(ref, c.act, 0.0), t.abs() + c.shift.double().abs().reshape(c.bs)


def add_emulate(c, mutation=None):
    s32 = c.a.float() + c.b.float()
    s = s32.to(c.dtype)
    v = (s32 if mutation == "unrounded_sum" else s.float()) * _chan_vec(c.scale, c, mutation)
    if mutation != "no_shift":
        v = v + _chan_vec(c.shift, c, mutation)
    return s, _act32(v, c.act, 0.0).to(c.dtype)


def _extra(act):
    return _SIGMOID_EXTRA if act == 3 else 0.0


# ---------------------------------------------------------------------------------------------- CPU proofs
def test_emulated_kernels_pass_the_checker_on_every_case():
    n = 0
    for c in affine_cases():
        ref, mag = affine_ref(c)
        check(affine_emulate(c), ref, mag, c.dtype, _extra(c.act), f"affine {c.shape} {c.dtype} act {c.act}")
        n += 1
    assert n == len(_SHAPES) * len(_DTYPES) * len(_PTRS) * len(_ACTS)
    for c in add_cases():
        s, ref, mag = add_ref(c)
        s2, y = add_emulate(c)
        assert torch.equal(s, s2)
        check(y, ref, mag, c.dtype, 0.0, f"add_affine {c.shape} {c.dtype} act {c.act}")


@pytest.mark.parametrize("mutation", ["chan_mod", "no_shift", "relu_before_res", "no_alpha"])
def test_checker_rejects_a_wrong_affine_act(mutation):
    """Every case whose arithmetic the mutation changes fails the checker (no case slips through)."""
    hit = 0
    for c in affine_cases():
        if not _applies(mutation, c):
            continue
        ref, mag = affine_ref(c)
        nbad, _ = violations(affine_emulate(c, mutation), ref, mag, c.dtype, _extra(c.act))
        assert nbad > 0, (mutation, c.shape, c.dtype, c.act)
        hit += 1
    assert hit >= 12, hit
    # the leaky and the clip form are both among the cases of no_alpha
    if mutation == "no_alpha":
        assert {c.act for c in affine_cases() if _applies(mutation, c)} == {2, 4}


@pytest.mark.parametrize("mutation", ["chan_mod", "no_shift", "unrounded_sum"])
def test_checker_rejects_a_wrong_add_affine_act(mutation):
    """``unrounded_sum`` (the affine applied to the fp32 sum instead of the sum as stored) differs from the
    right kernel by at most half a unit of the storage type times the scale, and only for fp16 / bf16 (an fp32
    sum is already the stored sum): it has to fail wherever there are enough elements for the two roundings to
    line up, here every 16-bit case of at least 128 elements."""
    hit = 0
    for c in add_cases():
        C, HW = _chw(c.shape)
        if mutation == "chan_mod" and (c.nhwc or HW == 1 or C == 1):
            continue
        if mutation == "unrounded_sum" and (c.dtype == torch.float32 or c.a.numel() < 128):
            continue
        s, ref, mag = add_ref(c)
        nbad, _ = violations(add_emulate(c, mutation)[1], ref, mag, c.dtype)
        assert nbad > 0, (mutation, c.shape, c.dtype, c.act)
        hit += 1
    assert hit >= 8, hit


# ---------------------------------------------------------------------------------------------- GPU helpers
def _nn():
    from synapseml_amd.ops import native

    return native.load("_nn")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, nhwc):
    """Device tensor with the case's memory layout (fresh allocation: 16-byte aligned)."""
    if t is None:
        return None
    d = t.cuda()
    d = d.contiguous(memory_format=torch.channels_last) if nhwc else d.contiguous()
    assert d.data_ptr() % 16 == 0
    return d


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _run_affine(c, inplace=False):
    nn = _nn()
    x, res = _dev(c.x, c.nhwc), _dev(c.res, c.nhwc)
    sc = None if c.scale is None else c.scale.cuda()
    sh = None if c.shift is None else c.shift.cuda()
    y = x if inplace else torch.full_like(x, float("nan"))
    C, HW = _chw(c.shape)
    nn.affine_act(x.data_ptr(), x.numel(), C, HW, c.nhwc, _ptr(sc), _ptr(sh), _ptr(res), c.act, float(c.alpha),
                  _DT[c.dtype], y.data_ptr(), _stream())
    torch.cuda.synchronize()
    return y.cpu()


@gpu
@pytest.mark.parametrize("shape", _SHAPES, ids=_shape_id)
def test_affine_act_matches_fp64(shape):
    """Every dtype x pointer combination x activation at this shape, within the derived bound. Sigmoid
    (the fast exponential) gets 2e-6 on top, |pre-activation| <= 19; its largest error on MI355X over all
    nine shapes is 1.09e-7 (fp32 outputs, at NHWC [2,64,7,7]; the other shapes 6.9e-8 to 8.8e-8)."""
    worst_sig = 0.0
    for c in affine_cases([shape]):
        ref, mag = affine_ref(c)
        y = _run_affine(c)
        if c.act == 3 and c.dtype == torch.float32:
            worst_sig = max(worst_sig, violations(y, ref, mag, c.dtype, _SIGMOID_EXTRA)[1])
        check(y, ref, mag, c.dtype, _extra(c.act),
              f"{_shape_id(shape)} {c.dtype} ptrs {[t is not None for t in (c.scale, c.shift, c.res)]} act {c.act}")
    print(f"sigmoid fp32 largest error at {_shape_id(shape)}: {worst_sig:.3e}")


@gpu
@pytest.mark.parametrize("dtype", _DTYPES, ids=str)
def test_affine_act_in_place(dtype):
    """y aliasing x, as the conv fallback's epilogue runs it."""
    for nhwc, shape in (_SHAPES[0], _SHAPES[4]):
        c = make_case(nhwc, shape, dtype, (1, 1, 1), 1, 0.0, 77)
        ref, mag = affine_ref(c)
        check(_run_affine(c, inplace=True), ref, mag, dtype, 0.0, f"in place {_shape_id((nhwc, shape))}")


@gpu
@pytest.mark.parametrize("shape", _SHAPES, ids=_shape_id)
def test_add_affine_act_matches_fp64(shape):
    """sum_out is the correctly rounded sum, bitwise; act_out the affine of that rounded sum."""
    nn = _nn()
    for c in add_cases([shape]):
        a, b = _dev(c.a, c.nhwc), _dev(c.b, c.nhwc)
        sc, sh = c.scale.cuda(), c.shift.cuda()
        s, y = torch.full_like(a, float("nan")), torch.full_like(a, float("nan"))
        C, HW = _chw(c.shape)
        nn.add_affine_act(a.data_ptr(), b.data_ptr(), a.numel(), C, HW, c.nhwc, sc.data_ptr(), sh.data_ptr(), c.act,
                          _DT[c.dtype], s.data_ptr(), y.data_ptr(), _stream())
        torch.cuda.synchronize()
        want_s, ref, mag = add_ref(c)
        assert torch.equal(s.cpu(), want_s), (shape, c.dtype)
        check(y.cpu(), ref, mag, c.dtype, 0.0, f"add_affine {_shape_id(shape)} {c.dtype} act {c.act}")


# ---------------------------------------------------------------------------------------------- max pool
_POOLS = [
    (2, 8, 1, 1, 3, 3, 1, 1, 1, 1),
    (1, 16, 2, 5, 3, 3, 2, 2, 1, 1),
    (1, 8, 7, 7, 3, 3, 1, 1, 1, 1),
    (1, 8, 9, 9, 3, 3, 3, 3, 0, 0),
    (2, 8, 6, 10, 3, 3, 2, 1, 1, 0),
    (1, 8, 5, 7, 2, 3, 1, 2, 0, 1),
    (1, 24, 4, 4, 5, 5, 1, 1, 2, 2),
    (1, 8, 3, 3, 1, 1, 2, 2, 0, 0),
    (3, 40, 13, 11, 2, 2, 2, 2, 0, 0),
]
_POOLS_WITH_EPILOGUE = (_POOLS[2], _POOLS[5])


def _pool_ref(x, geo):
    """max_pool2d of the same values in fp64 on the CPU (max is exact, so the cast back is too)."""
    _, _, _, _, kh, kw, sh, sw, ph, pw = geo
    return torch.nn.functional.max_pool2d(x.double().cpu(), (kh, kw), (sh, sw), (ph, pw))


def _run_pool(x, geo, shift=None, relu=0):
    n, c, h, w, kh, kw, sh, sw, ph, pw = geo
    assert tuple(x.shape) == (n, c, h, w) and c % 8 == 0 and x.is_contiguous(memory_format=torch.channels_last)
    assert x.data_ptr() % 16 == 0
    oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    y = torch.full((n, c, oh, ow), float("nan"), dtype=x.dtype, device="cuda").contiguous(memory_format=torch.channels_last)
    _nn().maxpool_nhwc(x.data_ptr(), n, h, w, c, kh, kw, sh, sw, ph, pw, oh, ow, _DT[x.dtype], y.data_ptr(), _stream(),
                       _ptr(shift), relu)
    torch.cuda.synchronize()
    return y.cpu()


def _same(y, ref):
    """Bitwise-equal values, NaN equal to NaN."""
    return y.shape == ref.shape and torch.equal(torch.nan_to_num(y.double(), nan=1e300), torch.nan_to_num(ref.double(), nan=1e300))


@gpu
@pytest.mark.parametrize("dtype", _DTYPES, ids=str)
@pytest.mark.parametrize("geo", _POOLS, ids=lambda g: "-".join(map(str, g)))
def test_maxpool_nhwc_geometries(geo, dtype):
    g = torch.Generator().manual_seed(sum(geo))
    x = torch.randn(geo[:4], generator=g).to(dtype)
    xd = _dev(x, 1)
    ref = _pool_ref(x, geo)
    y = _run_pool(xd, geo)
    assert tuple(y.shape) == tuple(ref.shape)
    assert torch.equal(y.double(), ref)
    if geo in _POOLS_WITH_EPILOGUE:
        # bias + ReLU of the producing conv moved past the pool: bitwise the unfused order
        b = torch.randn(geo[1], generator=g)
        unfused = _pool_ref(torch.relu(x.float() + b.view(1, -1, 1, 1)).to(dtype), geo)
        y2 = _run_pool(xd, geo, shift=b.cuda(), relu=1)
        assert torch.equal(y2.double(), unfused)
        y3 = _run_pool(xd, geo, shift=b.cuda(), relu=0)
        assert torch.equal(y3.double(), _pool_ref((x.float() + b.view(1, -1, 1, 1)).to(dtype), geo))


@gpu
@pytest.mark.parametrize("dtype", _DTYPES, ids=str)
@pytest.mark.parametrize("k", [3, 2], ids=["window3", "runtime-window"])
def test_maxpool_nhwc_infinities(k, dtype):
    """-inf, +inf and the largest finite value; a window of nothing but -inf gives -inf."""
    hw = 3 * k
    geo = (1, 8, hw, hw, k, k, k, k, 0, 0)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(geo[:4], generator=g).to(dtype)
    big = torch.finfo(dtype).max
    x[:, :, :k, :k] = -math.inf              # window (0, 0): all -inf
    x[:, :, 0, k + 1] = math.inf             # window (0, 1): holds +inf
    x[:, :, k:2 * k, :k] = -math.inf         # window (1, 0): -inf and the largest finite value
    x[:, :, k, 0] = big
    x[:, :, 2 * k, 2 * k] = -big             # window (2, 2): the most negative finite value among ordinary ones
    y = _run_pool(_dev(x, 1), geo)
    assert torch.equal(y.double(), _pool_ref(x, geo))
    assert torch.isneginf(y[:, :, 0, 0]).all() and torch.isposinf(y[:, :, 0, 1]).all()
    assert (y[:, :, 1, 0].double() == big).all()
    # padded cells never win over -inf either (3x3 / 1 pad 1 clamps its tap addresses into the image)
    geo_p = (1, 8, hw, hw, 3, 3, 1, 1, 1, 1)
    assert torch.equal(_run_pool(_dev(x, 1), geo_p).double(), _pool_ref(x, geo_p))


class _RT:
    """The little of the executor's per-node runtime the op functions read."""

    def __init__(self, nn, n_out=1):
        self.session = types.SimpleNamespace(_nn=nn)
        self.node_outputs = ["y", "idx"][:n_out]
        self.device = torch.device("cuda")


@gpu
@pytest.mark.parametrize("dtype", _DTYPES, ids=str)
@pytest.mark.parametrize("geo", [(1, 8, 6, 6, 3, 3, 1, 1, 1, 1), (1, 8, 6, 6, 2, 2, 2, 2, 0, 0)],
                         ids=["window3", "runtime-window"])
def test_maxpool_nhwc_propagates_nan(geo, dtype):
    """A NaN inside a window is the window's result, as in torch and ONNX Runtime; the kernel and the torch
    path of the MaxPool op agree, with and without the fused bias + ReLU."""
    from synapseml_amd.onnx import ops as O

    g = torch.Generator().manual_seed(9)
    x = torch.randn(geo[:4], generator=g).to(dtype)
    x[0, 0, 2, 3] = math.nan
    x[0, 3, 0, 0] = math.nan      # a corner: reached only by windows that also hold padding
    x[0, 5, 5, 5] = math.nan
    x[0, 5, 4, 4] = math.inf      # +inf next to a NaN: NaN still wins
    xd = _dev(x, 1)
    ref = _pool_ref(x, geo)
    assert torch.isnan(ref).any() and not torch.isnan(ref).all()
    assert _same(_run_pool(xd, geo), ref)
    b = torch.randn(geo[1], generator=g)
    at = {"kernel_shape": list(geo[4:6]), "strides": list(geo[6:8]), "pads": [geo[8], geo[9], geo[8], geo[9]]}
    for inputs, attrs in (([xd], at), ([xd, b.cuda()], dict(at, __act=1))):
        calls = []
        real = _nn()
        spy = types.SimpleNamespace(maxpool_nhwc=lambda *a, **k: calls.append(1) or real.maxpool_nhwc(*a, **k))
        yk = O.OPS["MaxPool"](_RT(spy), attrs, inputs)[0]
        yt = O.OPS["MaxPool"](_RT(None), attrs, inputs)[0]
        torch.cuda.synchronize()
        assert calls == [1]
        assert _same(yk.cpu(), yt.cpu())
        assert torch.isnan(yk).sum().item() == torch.isnan(ref).sum().item()


# ---------------------------------------------------------------------------------------------- global average pool
@gpu
@pytest.mark.parametrize("dtype", _DTYPES, ids=str)
@pytest.mark.parametrize("N,HW,C", [(1, 1, 8), (3, 49, 40), (2, 9, 3), (5, 12, 257), (1, 1000, 16)])
def test_gap_nhwc_matches_fp64(N, HW, C, dtype):
    """Bound of a sequential fp32 sum and one rounding: 0.5 * spacing_T(ref) + HW * 2^-24 * mean|x|."""
    g = torch.Generator().manual_seed(N * 1000 + HW + C)
    x = (torch.randn(N, HW, C, generator=g) + 0.5).to(dtype)
    xd = x.cuda()
    y = torch.full((N, C), float("nan"), dtype=dtype, device="cuda")
    _nn().gap_nhwc(xd.data_ptr(), N, HW, C, _DT[dtype], y.data_ptr(), _stream())
    torch.cuda.synchronize()
    ref = x.double().mean(1)
    tol = 0.5 * spacing(ref, dtype) + HW * _U32 * x.double().abs().mean(1)
    err = (y.cpu().double() - ref).abs()
    assert bool((err <= tol).all()), (float(err.max()), float((err / tol).max()))


# ---------------------------------------------------------------------------------------------- softmax_rows
_SOFTMAX_SHAPES = [(1, 1), (5, 63), (4, 64), (3, 65), (7, 1000), (9, 2)]


def _run_softmax(x, want_y=True, want_amax=True):
    rows, cols = x.shape
    xd = x.cuda().contiguous()
    y = torch.full((rows, cols), float("nan"), device="cuda") if want_y else None
    am = torch.full((rows,), -7, dtype=torch.int64, device="cuda") if want_amax else None
    _nn().softmax_rows(xd.data_ptr(), rows, cols, _ptr(y), _ptr(am), _stream())
    torch.cuda.synchronize()
    return (None if y is None else y.cpu()), (None if am is None else am.cpu())


def _softmax_inputs(rows, cols, seed):
    """x - max >= -28 (clamped at +-14): the fast exponential loses about |x - max| * 2^-24 in its argument."""
    g = torch.Generator().manual_seed(seed)
    return (4 * torch.randn(rows, cols, generator=g)).clamp(-14, 14)


def _rel_err(y, ref):
    nz = ref > 0
    assert bool((y.double()[~nz] == 0).all())
    return float(((y.double()[nz] - ref[nz]).abs() / ref[nz]).max()) if nz.any() else 0.0


def _check_softmax(x, what):
    """All three output combinations; argmax exact; values within 8x the error of torch.softmax in fp32 on the
    device (against fp64); each row sums to 1 within (cols / 64 + 8) * 2^-23. Returns (torch, kernel) errors."""
    rows, cols = x.shape
    ref = torch.softmax(x.double(), 1)
    want = torch.from_numpy(np.argmax(x.double().numpy(), 1))
    y, am = _run_softmax(x)
    y_only, none_am = _run_softmax(x, want_amax=False)
    none_y, am_only = _run_softmax(x, want_y=False)
    assert none_am is None and none_y is None
    assert torch.equal(y, y_only) and torch.equal(am, am_only)
    assert torch.equal(am, want), (what, am.tolist(), want.tolist())
    assert bool(torch.isfinite(y).all()), what
    e_torch = _rel_err(torch.softmax(x.cuda(), 1).cpu(), ref)
    e_kernel = _rel_err(y, ref)
    print(f"softmax {what}: torch fp32 rel err {e_torch:.3e}, kernel {e_kernel:.3e}")
    assert e_kernel <= 8 * e_torch, (what, e_kernel, e_torch)
    assert float((y.double().sum(1) - 1).abs().max()) <= (cols / 64 + 8) * 2.0 ** -23, what
    return e_torch, e_kernel


@gpu
@pytest.mark.parametrize("rows,cols", _SOFTMAX_SHAPES)
def test_softmax_rows_matches_fp64(rows, cols):
    """The gate is 8x the error of torch.softmax on the same inputs. Largest relative error against fp64 on
    MI355X, at (7,1000): torch.softmax (fp32, device) 1.15e-6, the kernel 2.45e-6. Per shape, torch / kernel:
    (1,1) 0 / 0, (5,63) 9.95e-7 / 1.77e-6, (4,64) 1.02e-6 / 1.56e-6, (3,65) 9.32e-7 / 1.87e-6, (9,2) 2.10e-7 /
    2.34e-7."""
    _check_softmax(_softmax_inputs(rows, cols, 31 * rows + cols), f"({rows},{cols})")


@gpu
def test_softmax_rows_offset_and_minus_inf():
    """Rows with a large common offset and rows holding -inf entries stay finite and right."""
    x = _softmax_inputs(6, 200, 3)
    x[:3] = x[:3] / 4 + 1e4
    x[3, ::3] = -math.inf
    x[4, :199] = -math.inf        # one finite entry, in the last column
    x[5, 1:] = -math.inf          # one finite entry, in the first
    _check_softmax(x, "offset / -inf")
    y, am = _run_softmax(x)
    assert am[4].item() == 199 and am[5].item() == 0 and y[4, 199].item() == 1.0 and y[5, 0].item() == 1.0


@gpu
def test_softmax_rows_ties_go_to_the_lowest_index():
    x = _softmax_inputs(6, 200, 4).clamp(max=10)
    for r, cols in enumerate([(70, 134), (134, 70, 198), (5, 6), (64, 63), (199, 0), (128, 129, 65)]):
        x[r, list(cols)] = 12.0   # the maximum, repeated 64 apart (one lane) and 1 apart (neighbouring lanes)
    _, am = _run_softmax(x, want_y=False)
    assert am.tolist() == [70, 70, 5, 63, 0, 65]
    assert am.tolist() == np.argmax(x.double().numpy(), 1).tolist()
    two = torch.tensor([[1.0, 1.0], [2.0, 1.0], [1.0, 2.0]])
    assert _run_softmax(two, want_y=False)[1].tolist() == [0, 0, 1]
    same = torch.zeros(3, 130)    # every lane ties
    assert _run_softmax(same, want_y=False)[1].tolist() == [0, 0, 0]


@gpu
def test_softmax_rows_nan_row_returns_the_first_nan():
    """As numpy and torch: the argmax of a row holding NaN is its first NaN, an index inside [0, cols)."""
    x = _softmax_inputs(7, 200, 5)
    for r, cols in enumerate([(130,), (7, 71), (71, 7, 135), (199,), (0,), (64, 65)]):
        x[r, list(cols)] = math.nan
    x[5, 3] = math.inf            # a larger number before the NaN does not hide it
    _, am = _run_softmax(x, want_y=False)
    want = np.argmax(x.numpy(), 1).tolist()
    assert want[:6] == [130, 7, 7, 199, 0, 64]
    assert am.tolist() == want and all(0 <= i < 200 for i in am.tolist())
    y, am2 = _run_softmax(x)
    assert torch.equal(am, am2)
    assert torch.isnan(y[:6]).all() and torch.isfinite(y[6]).all()
    one = torch.tensor([[math.nan]])
    assert _run_softmax(one, want_y=False)[1].tolist() == [0]


# ---------------------------------------------------------------------------------------------- float conv routes
_CONV_TOL = {torch.float32: 1e-5, torch.float16: 4e-3, torch.bfloat16: 3e-2}  # tests/test_gemm_gpu.py::_check
_PRECISION = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}

# name -> (C, Cout, groups, the _nn entry that must run it)
_ROUTES = {
    "tiled": (64, 64, 1, "conv_mfma"),
    "im2col": (24, 40, 1, "gemm"),
    "depthwise": (32, 32, 32, "group_conv"),
    "narrow-groups": (16, 16, 4, "group_conv"),
    "batched-gemm": (64, 128, 4, "gemm"),
}
# name -> (H, W, kernel, ONNX attributes)
_GEOMETRIES = {
    "dil2-pad2": (11, 14, (3, 3), {"dilations": [2, 2], "pads": [2, 2, 2, 2]}),
    "dil-1-2": (11, 14, (3, 3), {"dilations": [1, 2]}),
    "same-upper-s2": (12, 14, (3, 3), {"strides": [2, 2], "auto_pad": "SAME_UPPER"}),
    "same-lower-s2": (12, 14, (3, 3), {"strides": [2, 2], "auto_pad": "SAME_LOWER"}),
    "pads-1-0-2-1": (11, 14, (3, 3), {"pads": [1, 0, 2, 1]}),
    "k1x3": (11, 14, (1, 3), {}),
    "k3x1": (11, 14, (3, 1), {}),
    "stride-2-1": (11, 14, (3, 3), {"strides": [2, 1]}),
    "3x3-on-3x3": (3, 3, (3, 3), {}),
}


def _onnx_pads(attrs, hw, kernel):
    """(top, left, bottom, right) by the ONNX rules, worked out here independently of the executor."""
    st, dl = attrs.get("strides", [1, 1]), attrs.get("dilations", [1, 1])
    auto = attrs.get("auto_pad", "NOTSET")
    if auto == "NOTSET":
        return tuple(attrs.get("pads", [0, 0, 0, 0]))
    lo, hi = [], []
    for i in range(2):
        out = -(-hw[i] // st[i])
        total = max(0, (out - 1) * st[i] + (kernel[i] - 1) * dl[i] + 1 - hw[i])
        small, large = total // 2, total - total // 2
        lo.append(small if auto == "SAME_UPPER" else large)   # SAME_UPPER: the odd cell goes to the end
        hi.append(large if auto == "SAME_UPPER" else small)
    return lo[0], lo[1], hi[0], hi[1]


def _conv_ref(x, w, b, attrs, groups, dtype):
    """conv2d in fp64 on the CPU of the operands as stored (rounded to ``dtype``), explicit padding."""
    pt, pl, pb, pr = _onnx_pads(attrs, x.shape[2:], w.shape[2:])
    xp = torch.nn.functional.pad(x.to(dtype).double(), (pl, pr, pt, pb))
    return torch.nn.functional.conv2d(xp, w.to(dtype).double(), None if b is None else b.double(),
                                      stride=attrs.get("strides", [1, 1]), dilation=attrs.get("dilations", [1, 1]),
                                      groups=groups)


def _check_conv(y, ref, dtype, what=""):
    err = (torch.as_tensor(y).double().cpu() - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1.0)
    assert err <= _CONV_TOL[dtype] * scale, (what, err, scale, dtype)


def _count_nn(monkeypatch):
    """Count the launches of each conv entry of ``_nn`` (``gemm`` only with an implicit-im2col operand)."""
    nn = _nn()
    calls = {"conv_mfma": 0, "gemm": 0, "group_conv": 0}

    def wrap(name):
        real = getattr(nn, name)

        def f(*a, **k):
            if name != "gemm" or (len(a) >= 2 and isinstance(a[-2], (list, tuple)) and len(a[-2]) > 0):
                calls[name] += 1
            return real(*a, **k)

        monkeypatch.setattr(nn, name, f)

    for name in calls:
        wrap(name)
    return calls


def test_same_pads_of_a_stride_2_conv_on_an_even_size():
    """The MobileNet-style export: SAME_UPPER pads only the end, SAME_LOWER only the beginning."""
    from synapseml_amd.onnx.ops import conv_args

    at = {"strides": [2, 2], "auto_pad": "SAME_UPPER"}
    assert _onnx_pads(at, (12, 14), (3, 3)) == (0, 0, 1, 1)
    assert _onnx_pads(dict(at, auto_pad="SAME_LOWER"), (12, 14), (3, 3)) == (1, 1, 0, 0)
    for auto in ("SAME_UPPER", "SAME_LOWER"):
        a = dict(at, auto_pad=auto)
        _, _, _, pb, pe = conv_args(a, (2, 8, 12, 14), (8, 8, 3, 3))
        assert (pb[0], pb[1], pe[0], pe[1]) == _onnx_pads(a, (12, 14), (3, 3))


@gpu
@pytest.mark.parametrize("geometry", list(_GEOMETRIES))
@pytest.mark.parametrize("route", list(_ROUTES))
def test_conv_geometry_on_every_route(route, geometry, monkeypatch):
    """One-node Conv graphs through the GPU session, fp32 / fp16 / bf16, against fp64 conv2d; the kernel the
    route documents is the one that ran."""
    from synapseml_amd.onnx import InferenceSession, proto as P
    from synapseml_amd.onnx.writer import GraphBuilder

    C, Cout, groups, entry = _ROUTES[route]
    H, W, kernel, attrs = _GEOMETRIES[geometry]
    g = torch.Generator().manual_seed(len(route) * 100 + len(geometry))
    x = torch.randn(2, C, H, W, generator=g)
    cg = C // groups
    w = torch.randn(Cout, cg, *kernel, generator=g) / (kernel[0] * kernel[1] * cg) ** 0.5
    b = torch.randn(Cout, generator=g)
    gb = GraphBuilder("conv")
    gb.input("x", P.FLOAT32, [2, C, H, W])
    at = dict(attrs, kernel_shape=list(kernel), group=groups)
    gb.add("Conv", ["x", gb.init("w", w.numpy()), gb.init("b", b.numpy())], at, out="y")
    gb.output("y", P.FLOAT32, None)
    data = gb.to_bytes()
    calls = _count_nn(monkeypatch)
    for dtype in _DTYPES:
        for k in calls:
            calls[k] = 0
        sess = InferenceSession(data, device="cuda", precision=_PRECISION[dtype], use_graph=False)
        y = sess.run(None, {"x": x.numpy()})[0]
        ref = _conv_ref(x, w, b, attrs, groups, dtype)
        assert tuple(y.shape) == tuple(ref.shape), (y.shape, ref.shape)
        _check_conv(torch.from_numpy(np.asarray(y, dtype=np.float64)), ref, dtype, f"{route} {geometry}")
        assert calls == {k: int(k == entry) for k in calls}, (route, geometry, dtype, calls)


def _general(x, w, b, dtype, stride=(1, 1), pad=(1, 1, 1, 1), dil=(1, 1), groups=1, relu=0, res=None):
    from synapseml_amd.ops.conv import conv2d_nhwc_general

    xd = x.to("cuda", dtype).contiguous(memory_format=torch.channels_last)
    wp = w.to("cuda", dtype).permute(0, 2, 3, 1).contiguous()
    rd = None if res is None else res.to("cuda", dtype).contiguous(memory_format=torch.channels_last)
    y = conv2d_nhwc_general(xd, wp, w.shape[2], w.shape[3], stride, pad, dil, groups=groups,
                            bias=None if b is None else b.cuda(), relu=relu, res=rd)
    torch.cuda.synchronize()
    return y


@gpu
@pytest.mark.parametrize("dtype", _DTYPES, ids=str)
@pytest.mark.parametrize("C,Cout,groups", [(16, 16, 8), (32, 32, 32), (16, 32, 4)],
                         ids=["groups8-cg2", "depthwise", "groups4-cg4"])
def test_direct_conv_epilogues(C, Cout, groups, dtype, monkeypatch):
    """The direct kernel (narrow 3x3 groups, depthwise), bf16 included: bias present and absent, relu 0 / 1 /
    2, with and without a residual; odd output size, several blocks."""
    calls = _count_nn(monkeypatch)
    g = torch.Generator().manual_seed(C + Cout + groups)
    x = torch.randn(3, C, 13, 9, generator=g)
    w = torch.randn(Cout, C // groups, 3, 3, generator=g) / (9 * C // groups) ** 0.5
    bias = torch.randn(Cout, generator=g)
    res = torch.randn(3, Cout, 13, 9, generator=g)
    n = 0
    for b, relu, r in itertools.product((bias, None), (0, 1, 2), (None, res)):
        y = _general(x, w, b, dtype, groups=groups, relu=relu, res=r)
        ref = torch.nn.functional.conv2d(x.to(dtype).double(), w.to(dtype).double(), None if b is None else b.double(),
                                         padding=1, groups=groups)
        rr = None if r is None else r.to(dtype).double()
        if relu == 1:
            ref = torch.relu(ref)
        if rr is not None:
            ref = ref + rr
        if relu == 2:
            ref = torch.relu(ref)
        _check_conv(y, ref, dtype, f"bias {b is not None} relu {relu} res {r is not None}")
        n += 1
    assert calls == {"conv_mfma": 0, "gemm": 0, "group_conv": n}


@gpu
def test_direct_conv_second_trip_of_the_grid_stride_loop(monkeypatch):
    """More outputs than the capped grid has threads (2^16 blocks x 256): the loop's second trip. Small
    integers, so every product and sum is exact in fp16 and the result is bitwise the CPU's."""
    calls = _count_nn(monkeypatch)
    B, C, H, W = 2, 32, 520, 512
    assert B * C * H * W > 2 ** 24
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-2, 3, (B, C, H, W), generator=g).float()
    w = torch.randint(-2, 3, (C, 1, 3, 3), generator=g).float()
    b = torch.randint(-3, 4, (C,), generator=g).float()
    y = _general(x, w, b, torch.float16, groups=C)
    ref = torch.nn.functional.conv2d(x, w, b, padding=1, groups=C)  # |values| <= 39: exact in fp32 and fp16
    assert calls == {"conv_mfma": 0, "gemm": 0, "group_conv": 1}
    assert torch.equal(y.cpu(), ref.half())


# ---------------------------------------------------------------------------------------------- dispatch guards
class _Recorder:
    """Stands in for ``_nn``: records what would have been launched and launches nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: self.calls.append((name, a, k))


def _affine64(x, scale, shift, res, act):
    bs = _bshape(x.shape)
    v = x.double().cpu() * scale.double().cpu().reshape(bs) + shift.double().cpu().reshape(bs)
    if res is not None:
        v = v + res.double().cpu()
    return torch.relu(v) if act == 1 else v


def _mag(x, scale, shift, res):
    bs = _bshape(x.shape)
    m = (x.double().cpu() * scale.double().cpu().reshape(bs)).abs() + shift.double().cpu().abs().reshape(bs)
    return m if res is None else m + res.double().cpu().abs()


@gpu
@pytest.mark.parametrize("dtype", _DTYPES, ids=str)
@pytest.mark.parametrize("nhwc", [1, 0])
def test_broadcast_residual_is_expanded_before_the_kernel(nhwc, dtype):
    """A [1, C, 1, 1] residual against [N, C, H, W]: the kernel reads one residual element per element of x,
    so the residual's own buffer must never be what it gets."""
    from synapseml_amd.onnx import session as S

    g = torch.Generator().manual_seed(21)
    x = _dev(torch.randn(2, 16, 5, 4, generator=g).to(dtype), nhwc)
    r = torch.randn(1, 16, 1, 1, generator=g).to(dtype).cuda()
    sc, sh = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g)
    rec = _Recorder()
    S._affine_act(_RT(rec), x, sc, sh, r, 1, 0.0)
    for name, a, _ in rec.calls:
        assert name == "affine_act"
        assert a[7] != r.data_ptr() and a[7] != 0, "the 16-element residual reached a kernel that reads 640"
    y = S._affine_act(_RT(_nn()), x, sc, sh, r, 1, 0.0)
    torch.cuda.synchronize()
    assert y.shape == x.shape
    check(y, _affine64(x, sc, sh, r, 1), _mag(x, sc, sh, r).expand(x.shape), dtype, 0.0, "broadcast residual")
    # a residual of the right shape in the other layout is converted, not read as it lies
    r2 = _dev(torch.randn(2, 16, 5, 4, generator=g).to(dtype), 1 - nhwc)
    y2 = S._affine_act(_RT(_nn()), x, sc, sh, r2, 1, 0.0)
    torch.cuda.synchronize()
    check(y2, _affine64(x, sc, sh, r2, 1), _mag(x, sc, sh, r2), dtype, 0.0, "residual in the other layout")


def _misaligned(t):
    """The same values at an address that is no multiple of 16."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@gpu
@pytest.mark.parametrize("dtype", _DTYPES, ids=str)
def test_misaligned_tensors_take_the_torch_path(dtype):
    from synapseml_amd.onnx import ops as O, session as S

    g = torch.Generator().manual_seed(22)
    x = torch.randn(2, 8, 4, 6, generator=g).to(dtype).cuda()
    r = torch.randn(2, 8, 4, 6, generator=g).to(dtype).cuda()
    sc, sh = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    rec = _Recorder()
    rt = _RT(rec)
    for xx, rr in ((_misaligned(x), r), (x, _misaligned(r)), (_misaligned(x), None)):
        y = S._affine_act(rt, xx, sc.cuda(), sh.cuda(), rr, 1, 0.0)
        assert rec.calls == []
        check(y, _affine64(x, sc, sh, None if rr is None else r, 1), _mag(x, sc, sh, None if rr is None else r), dtype)
    for aa, bb in ((_misaligned(x), r), (x, _misaligned(r))):
        s, y = S._fused_add_affine_act(rt, {"__act": 1}, [aa, bb, sc.cuda(), sh.cuda()])
        assert rec.calls == []
        want_s = (x.float() + r.float()).to(dtype)
        assert torch.equal(s, want_s)
        check(y, _affine64(want_s, sc, sh, None, 1), _mag(want_s, sc, sh, None), dtype)
    # MaxPool: a channels-last view that starts one element into its buffer
    buf = torch.randn(2 * 6 * 6 * 8 + 1, generator=g).to(dtype).cuda()
    xp = buf[1:].view(2, 6, 6, 8).permute(0, 3, 1, 2)
    assert xp.data_ptr() % 16 != 0 and xp.is_contiguous(memory_format=torch.channels_last)
    at = {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1]}
    y = O.OPS["MaxPool"](rt, at, [xp])[0]
    assert rec.calls == []
    assert torch.equal(y.double().cpu(), _pool_ref(xp, (2, 8, 6, 6, 3, 3, 2, 2, 1, 1)))


@gpu
def test_maxpool_declines_what_the_kernel_does_not_do():
    """ceil_mode, dilation, asymmetric pads, an indices output and C % 8 != 0 run on torch, on the device,
    with the right values; the plain form of the same input goes to the kernel."""
    from synapseml_amd.onnx import ops as O

    g = torch.Generator().manual_seed(23)
    x8 = _dev(torch.randn(2, 8, 9, 10, generator=g), 1)
    x12 = _dev(torch.randn(2, 12, 9, 10, generator=g), 1)
    base = {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1]}
    F = torch.nn.functional
    ninf = -math.inf
    cases = [
        (x8, dict(base, ceil_mode=1), 1, lambda t: F.max_pool2d(t, 3, 2, 1, ceil_mode=True)),
        (x8, dict(base, dilations=[2, 2]), 1, lambda t: F.max_pool2d(t, 3, 2, 1, dilation=2)),
        (x8, dict(base, pads=[0, 1, 1, 0]), 1, lambda t: F.max_pool2d(F.pad(t, (1, 0, 0, 1), value=ninf), 3, 2)),
        (x8, base, 2, lambda t: F.max_pool2d(t, 3, 2, 1)),
        (x12, base, 1, lambda t: F.max_pool2d(t, 3, 2, 1)),
    ]
    for x, at, n_out, ref in cases:
        rec = _Recorder()
        out = O.OPS["MaxPool"](_RT(rec, n_out), at, [x])
        assert rec.calls == [], at
        assert out[0].is_cuda and len(out) == n_out
        assert torch.equal(out[0].double().cpu(), ref(x.double().cpu())), at
        if n_out == 2:
            want_idx = F.max_pool2d(x.double().cpu(), 3, 2, 1, return_indices=True)[1]
            assert torch.equal(out[1].cpu(), want_idx)
    rec = _Recorder()
    O.OPS["MaxPool"](_RT(rec), base, [x8])
    assert [c[0] for c in rec.calls] == ["maxpool_nhwc"]


@gpu
def test_add_affine_act_with_1d_operands():
    """No channel axis to index: the torch path, elementwise."""
    from synapseml_amd.onnx import session as S

    a = torch.arange(24, dtype=torch.float32, device="cuda") - 11
    b = torch.ones(24, device="cuda")
    sc, sh = torch.tensor([2.0], device="cuda"), torch.tensor([-3.0], device="cuda")
    rec = _Recorder()
    s, y = S._fused_add_affine_act(_RT(rec), {"__act": 1}, [a, b, sc, sh])
    assert rec.calls == []
    assert torch.equal(s, a + b) and s.shape == y.shape == (24,)
    assert torch.equal(y, torch.relu((a + b) * 2 - 3))
