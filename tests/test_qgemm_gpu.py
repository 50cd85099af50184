"""K18 int8 MFMA GEMM / conv (csrc/nn/qgemm_mfma.hip, ops.qgemm) against numpy int64: every comparison is
exact. Also the four ONNX operators on it, device session against host session."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NP = {"u8": np.uint8, "s8": np.int8}


def _Q():
    from synapseml_amd.ops import qgemm as Q

    return Q


def _rand(rng, kind, shape):
    lo, hi = (0, 256) if kind == "u8" else (-128, 128)
    return rng.integers(lo, hi, shape).astype(NP[kind])


def _dev(a):
    return None if a is None else torch.from_numpy(np.asarray(a)).cuda()


def _zps(rng, mode, ka, kb, M, N):
    if mode == "none":
        return None, None
    if mode == "scalar":
        return _rand(rng, ka, ()), _rand(rng, kb, ())
    return _rand(rng, ka, (M,)), _rand(rng, kb, (N,))


def _mm_ref(a, b, az, bz):
    af = a.astype(np.int64) - (0 if az is None else np.asarray(az, np.int64).reshape(-1, 1))
    bf = b.astype(np.int64) - (0 if bz is None else np.asarray(bz, np.int64).reshape(1, -1))
    return af @ bf


def _requant_ref(acc, mult, ys, yz):
    """(reference, it holds a tie, it holds both clamps)"""
    info = np.iinfo(yz.dtype)
    t = acc * mult / np.float64(ys)
    q = np.rint(t) + np.float64(yz)
    tie = (np.abs(t - np.floor(t)) == 0.5) & (q > info.min) & (q < info.max)
    ref = np.clip(q, info.min, info.max).astype(yz.dtype)
    return ref, tie.any(), (ref == info.min).any() and (ref == info.max).any()


@pytest.mark.parametrize("zp", ["none", "scalar", "vector"])
@pytest.mark.parametrize("b_nk", [False, True])  # B row-major [K][N], or a transposed view of [N][K]
@pytest.mark.parametrize("ka,kb", [("u8", "u8"), ("u8", "s8"), ("s8", "u8"), ("s8", "s8")])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (16, 16, 64), (64, 64, 128), (33, 48, 272), (65, 67, 129)])
def test_matmul_integer(M, N, K, ka, kb, b_nk, zp):
    rng = np.random.default_rng(M * 131 + N * 7 + K)
    a, b = _rand(rng, ka, (M, K)), _rand(rng, kb, (K, N))
    az, bz = _zps(rng, zp, ka, kb, M, N)
    bd = _dev(np.ascontiguousarray(b.T)).t() if b_nk else _dev(b)
    y = _Q().matmul_integer(_dev(a), bd, _dev(az), _dev(bz))
    assert y.dtype == torch.int32
    np.testing.assert_array_equal(y.cpu().numpy(), _mm_ref(a, b, az, bz))


def test_matmul_integer_batched_broadcast_b():
    rng = np.random.default_rng(5)
    a, b = _rand(rng, "u8", (3, 33, 272)), _rand(rng, "s8", (272, 48))
    az, bz = _rand(rng, "u8", (33,)), _rand(rng, "s8", (48,))
    y = _Q().matmul_integer(_dev(a), _dev(b), _dev(az), _dev(bz))
    np.testing.assert_array_equal(y.cpu().numpy(), np.stack([_mm_ref(a[i], b, az, bz) for i in range(3)]))


@pytest.mark.parametrize("az,bz", [(0, 0), (255, -128)])
def test_matmul_integer_extreme_k(az, bz):
    Q, K = _Q(), 32768
    a = torch.full((16, K), 255, dtype=torch.uint8, device="cuda")
    b = torch.full((K, 16), -128, dtype=torch.int8, device="cuda")
    zp = (_dev(np.array(az, np.uint8)), _dev(np.array(bz, np.int8)))
    y = Q.matmul_integer(a, b, *zp)
    np.testing.assert_array_equal(y.cpu().numpy(), np.full((16, 16), (255 - az) * (-128 - bz) * K, np.int64))
    a2 = torch.zeros((16, K + 1), dtype=torch.uint8, device="cuda")
    assert Q.supported(a, b, *zp) and not Q.supported(a2, torch.zeros((K + 1, 16), dtype=torch.int8, device="cuda"))


def _conv_ref(x, w, xz, wz, stride, pads, dil, group):
    xf = np.pad(x.astype(np.int64) - int(xz), ((0, 0), (0, 0), (pads[0], pads[2]), (pads[1], pads[3])))
    wf = w.astype(np.int64) - np.asarray(wz, np.int64).reshape(-1, 1, 1, 1)
    (B, _, H, W), (co, cg, R, S) = xf.shape, w.shape
    oh, ow = (H - dil * (R - 1) - 1) // stride + 1, (W - dil * (S - 1) - 1) // stride + 1
    out, ng = np.zeros((B, co, oh, ow), np.int64), co // group
    for g in range(group):
        for r in range(R):
            for s in range(S):
                p = xf[:, g * cg:(g + 1) * cg, r * dil:r * dil + stride * (oh - 1) + 1:stride,
                       s * dil:s * dil + stride * (ow - 1) + 1:stride]
                out[:, g * ng:(g + 1) * ng] += np.einsum("bchw,oc->bohw", p, wf[g * ng:(g + 1) * ng, :, r, s])
    return out


CONVS = [(1, 3, 7, 7, 5, 3, 1, (1, 1, 1, 1), 1, 1), (2, 16, 9, 8, 32, 3, 2, (0, 1, 1, 2), 1, 1),
         (1, 64, 6, 6, 64, 1, 1, (0, 0, 0, 0), 1, 1), (1, 8, 9, 9, 16, 3, 1, (2, 2, 2, 2), 2, 1),
         (1, 32, 5, 5, 32, 3, 1, (1, 1, 1, 1), 1, 2)]


@pytest.mark.parametrize("wz_vec", [False, True])
@pytest.mark.parametrize("xz", [0, 128, 37])
@pytest.mark.parametrize("case", CONVS)
def test_conv_integer(case, xz, wz_vec):
    B, C, H, W, co, R, st, pads, dil, group = case
    rng = np.random.default_rng(C * 17 + co + xz)
    x, w = _rand(rng, "u8", (B, C, H, W)), _rand(rng, "s8", (co, C // group, R, R))
    wz = _rand(rng, "s8", (co,)) if wz_vec else np.array(0, np.int8)
    y = _Q().conv_integer(_dev(x), _dev(w), _dev(np.array(xz, np.uint8)), _dev(wz), (st, st), pads, (dil, dil), group)
    assert y.dtype == torch.int32
    np.testing.assert_array_equal(y.cpu().numpy(), _conv_ref(x, w, xz, wz, st, pads, dil, group))


def _narrow(rng, kind, shape, zp):
    """values within 3 of the zero point: accumulators small enough that some requantised outputs stay in range"""
    return (int(zp) + rng.integers(-3, 4, shape)).astype(NP[kind])


def _scales(n):
    """a_s * b_s[n] / y_s is 0.5 on even columns (ties at odd accumulators) and 64 on odd ones (both clamps)"""
    return np.float32(1.0), np.where(np.arange(n) % 2 == 0, 0.25, 32.0).astype(np.float32), np.float32(0.5)


@pytest.mark.parametrize("yz", [np.uint8(128), np.int8(-3)])
def test_qlinear_matmul(yz):
    M, N, K = 33, 48, 272
    rng = np.random.default_rng(11)
    az, bz = np.uint8(37), np.int8(-5)
    a, b = _narrow(rng, "u8", (M, K), az), _narrow(rng, "s8", (K, N), bz)
    a_s, b_s, y_s = _scales(N)
    ref, ties, clamps = _requant_ref(_mm_ref(a, b, az, bz), np.float64(a_s) * b_s.astype(np.float64)[None], y_s, yz)
    assert ties and clamps
    y = _Q().qlinear_matmul(*map(_dev, (a, a_s, az, b, b_s, bz, y_s, yz)))
    np.testing.assert_array_equal(y.cpu().numpy(), ref)


@pytest.mark.parametrize("yz", [np.uint8(128), np.int8(-3)])
def test_qlinear_conv(yz):
    B, C, H, W, co, R, st, pads, dil, group = CONVS[1]
    rng = np.random.default_rng(12)
    xz, wz = np.uint8(37), rng.integers(-4, 5, (co,)).astype(np.int8)
    x = _narrow(rng, "u8", (B, C, H, W), xz)
    w = (wz[:, None, None, None] + rng.integers(-3, 4, (co, C, R, R))).astype(np.int8)
    bias = rng.integers(-40, 41, (co,)).astype(np.int32)
    x_s, w_s, y_s = _scales(co)
    acc = _conv_ref(x, w, xz, wz, st, pads, dil, group) + bias[None, :, None, None]
    ref, ties, clamps = _requant_ref(acc, np.float64(x_s) * w_s.astype(np.float64)[None, :, None, None], y_s, yz)
    assert ties and clamps
    y = _Q().qlinear_conv(*map(_dev, (x, x_s, xz, w, w_s, wz, y_s, yz, bias)), (st, st), pads, (dil, dil), group)
    np.testing.assert_array_equal(y.cpu().numpy(), ref)


def _graphs():
    rng = np.random.default_rng(13)
    a, b = _rand(rng, "u8", (33, 272)), _rand(rng, "s8", (272, 48))
    az, bz = np.array(12, np.uint8), _rand(rng, "s8", (48,))
    x, w = _rand(rng, "u8", (1, 3, 7, 7)), _rand(rng, "s8", (5, 3, 3, 3))
    xz, wz = np.array(100, np.uint8), _rand(rng, "s8", (5,))
    f = lambda v: np.array(v, np.float32)  # noqa: E731
    conv_at = {"kernel_shape": [3, 3], "pads": [1, 1, 1, 1]}
    return {
        "MatMulInteger": ([("A", a), ("B", b), ("az", az), ("bz", bz)], None),
        "QLinearMatMul": ([("A", a), ("as", f(0.02)), ("az", az), ("B", b), ("bs", f(0.05)), ("bz", bz),
                           ("ys", f(40.0)), ("yz", np.array(7, np.uint8))], None),
        "ConvInteger": ([("x", x), ("w", w), ("xz", xz), ("wz", wz)], conv_at),
        "QLinearConv": ([("x", x), ("xs", f(0.05)), ("xz", xz), ("w", w), ("ws", f([.01, .02, .03, .04, .05])),
                         ("wz", wz), ("ys", f(5.0)), ("yz", np.array(-9, np.int8)),
                         ("b", np.array([10, -20, 30, -40, 50], np.int32))], conv_at),
    }


@pytest.mark.parametrize("op_type", ["MatMulInteger", "QLinearMatMul", "ConvInteger", "QLinearConv"])
def test_onnx_operator_on_device(op_type, monkeypatch):
    from synapseml_amd.onnx import ops_ext
    from tests.test_onnx_ops_ext import run1

    inputs, attrs = _graphs()[op_type]
    (host,) = run1(op_type, inputs, attrs, device="cpu")

    def host_path(*a, **k):
        raise AssertionError("host path taken")

    monkeypatch.setattr(ops_ext, "_int_matmul", host_path)
    monkeypatch.setattr(ops_ext, "_conv_f64", host_path)
    (dev,) = run1(op_type, inputs, attrs, device="cuda")
    assert dev.dtype == host.dtype and dev.shape == host.shape
    np.testing.assert_array_equal(dev, host)
    monkeypatch.setenv("SML_QGEMM", "0")
    with pytest.raises(Exception, match="host path taken"):
        run1(op_type, inputs, attrs, device="cuda")
