"""K22 fused MFMA attention (csrc/nn/attn_mfma.hip, ops.attention) against fp64 numpy on the same fp16 / bf16
rounded inputs. Tolerance of the direct tests, derived: |out - ref| <= 2 u max|V| + 1e-6 with u = 2^-11 (fp16) or
2^-8 (bf16): one rounding of P inside the convex combination plus one rounding of the output; the fp32
accumulation terms are orders of magnitude below. The operator tests allow twice the error of the unfused path
on the same inputs, since the fp16 projection in front of the kernel rounds q, k and v."""
import gc
import math

import numpy as np
import pytest
import torch

from synapseml_amd.onnx import InferenceSession, ops_ext, proto as P
from synapseml_amd.onnx.writer import GraphBuilder
from synapseml_amd.ops import attention as A

pytestmark = pytest.mark.gpu
B, H = 2, 3
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SHAPES = [(1, 1, 32), (16, 16, 32), (17, 65, 64), (64, 64, 64), (65, 130, 128), (33, 129, 64)]


def _ref(q, k, v, heads, add=None, causal=False):
    """fp64 attention: q [B, S, D], k / v [B, L, D]; add broadcastable to [B, heads, S, L]"""
    (Bn, S, D), L, d = q.shape, k.shape[1], q.shape[2] // heads
    qh, kh, vh = (np.asarray(t, np.float64).reshape(Bn, -1, heads, d).transpose(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(0, 1, 3, 2) / math.sqrt(d)
    if add is not None:
        s = s + add
    if causal:
        s = np.where(np.tri(S, L, L - S, dtype=bool), s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    return ((p / p.sum(-1, keepdims=True)) @ vh).transpose(0, 2, 1, 3).reshape(Bn, S, D)


def _qkv(S, L, d, dtype, seed):
    """q, k (standard deviation 4: the row max moves between key tiles) and v as views of packed tensors"""
    g = torch.Generator().manual_seed(seed)
    D = H * d
    if S == L:
        q, k, v = torch.split((torch.randn(B, S, 3 * D, generator=g) * torch.tensor([4.0, 4.0, 1.0])
                               .repeat_interleave(D)).to("cuda", dtype), D, -1)
    else:
        q = (torch.randn(B, S, D, generator=g) * 4).to("cuda", dtype)
        k, v = torch.split((torch.randn(B, L, 2 * D, generator=g) * torch.tensor([4.0, 1.0])
                            .repeat_interleave(D)).to("cuda", dtype), D, -1)
    return q, k, v


def _check(q, k, v, out, **ref_args):
    ref = _ref(*(t.float().cpu().numpy() for t in (q, k, v)), H, **ref_args)
    bound = 2 * U[q.dtype] * float(v.float().abs().max()) + 1e-6
    err = float(np.abs(out.float().cpu().numpy() - ref).max())
    print(f"max err {err:.3e} = {err / (bound - 1e-6) * 2:.3f} u max|V| (bound {bound:.3e})")
    assert out.dtype == q.dtype and err <= bound


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("S,L,d", SHAPES)
def test_attention(S, L, d, dtype):
    q, k, v = _qkv(S, L, d, dtype, 1)
    assert q.stride(2) == 1 and (S != L or not q.is_contiguous())
    _check(q, k, v, A.attention(q, k, v, H))


@pytest.mark.parametrize("terms", ["key_add", "bias", "bias_bcast", "both"])
@pytest.mark.parametrize("S,L,d", [(33, 129, 64), (65, 130, 128)])
def test_additive_terms(S, L, d, terms):
    q, k, v = _qkv(S, L, d, torch.float16, 2)
    g = torch.Generator().manual_seed(3)
    key_add = bias = None
    add = 0.0
    if terms in ("key_add", "both"):  # from lengths; every batch entry keeps a valid key
        lens = torch.tensor([L, 1 + L // 3]).reshape(B, 1)
        key_add = torch.where(torch.arange(L).unsqueeze(0) < lens, 0.0, -10000.0).cuda()
        add = add + key_add.cpu().numpy().astype(np.float64).reshape(B, 1, 1, L)
    if terms != "key_add":
        bias = torch.randn(1 if terms == "bias_bcast" else B, H, S, L, generator=g).cuda()
        add = add + bias.cpu().numpy().astype(np.float64)
    _check(q, k, v, A.attention(q, k, v, H, key_add=key_add, bias=bias), add=add)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("S,L", [(64, 64), (17, 65), (65, 130)])
def test_causal(S, L, dtype):
    q, k, v = _qkv(S, L, 64, dtype, 4)
    _check(q, k, v, A.attention(q, k, v, H, causal=True), causal=True)


def _run_op(op_type, inputs, attrs, use_graph=False, runs=1):
    b = GraphBuilder(op_type)
    for name, arr in inputs:
        if name:
            b.input(name, P.ONNX_OF[arr.dtype], list(arr.shape))
    b.output(b.add(op_type, [n for n, _ in inputs], attrs, out="y", domain="com.microsoft"), P.FLOAT32, None)
    sess = InferenceSession(b.to_bytes(), device="cuda", precision="fp16", optimization_level="NO_OPT",
                            use_graph=use_graph)
    ys = [np.asarray(sess.run(None, {n: a for n, a in inputs if n})[0], np.float64) for _ in range(runs)]
    del sess  # a captured graph and its memory pool go here, with the device idle, not at a later collection
    gc.collect()
    torch.cuda.synchronize()
    return ys


def _op_check(monkeypatch, op_type, inputs, attrs, ref):
    """the kernel path (no fall-back: _attend raises) within twice the unfused path's error; graph replays equal
    the eager run"""
    monkeypatch.setenv("SML_ATTN", "0")
    parent = float(np.abs(_run_op(op_type, inputs, attrs)[0] - ref).max())
    monkeypatch.setenv("SML_ATTN", "1")
    monkeypatch.setattr(ops_ext, "_attend", lambda *a, **k: pytest.fail("fell back to _attend()"))
    eager = _run_op(op_type, inputs, attrs)[0]
    err = float(np.abs(eager - ref).max())
    print(f"{op_type}: kernel path max err {err:.3e}, unfused path {parent:.3e}")
    assert err <= 2 * parent
    for y in _run_op(op_type, inputs, attrs, use_graph=True, runs=3):
        np.testing.assert_array_equal(y, eager)


def _f16(a):
    return a.astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("unidirectional", [0, 1])
def test_attention_operator(monkeypatch, unidirectional):
    rng = np.random.default_rng(5)
    Bn, S, Pl, heads, d = 2, 17, 5, 2, 32
    D, L = heads * d, S + Pl
    x, w = _f16(rng.standard_normal((Bn, S, D))), _f16(rng.standard_normal((D, 3 * D)) * 0.2)
    wb, past = _f16(rng.standard_normal(3 * D) * 0.1), _f16(rng.standard_normal((2, Bn, heads, Pl, d)))
    mask = np.ones((Bn, L), np.int32)
    mask[1, 2:4] = 0
    q, k, v = np.split(x.astype(np.float64) @ w + wb, 3, -1)
    k, v = (np.concatenate([p.transpose(0, 2, 1, 3).reshape(Bn, Pl, D), t], 1) for p, t in ((past[0], k), (past[1], v)))
    ref = _ref(q, k, v, heads, np.where(mask > 0, 0.0, -10000.0).reshape(Bn, 1, 1, L), bool(unidirectional))
    _op_check(monkeypatch, "Attention", [("x", x), ("w", w), ("wb", wb), ("m", mask), ("past", past)],
              {"num_heads": heads, "unidirectional": unidirectional}, ref)


def test_multi_head_attention_operator(monkeypatch):
    rng = np.random.default_rng(6)
    Bn, S, L, heads, d = 2, 17, 40, 2, 32
    D = heads * d
    q, k, v = (_f16(rng.standard_normal((Bn, n, D))) for n in (S, L, L))
    bias, rb = _f16(rng.standard_normal(3 * D) * 0.1), rng.standard_normal((1, heads, S, L)).astype(np.float32)
    qb, kb, vb = (_f16(t.astype(np.float64) + bias[i * D:(i + 1) * D]) for i, t in enumerate((q, k, v)))  # the operator adds in fp16
    _op_check(monkeypatch, "MultiHeadAttention", [("q", q), ("k", k), ("v", v), ("b", bias), ("", None), ("rb", rb)],
              {"num_heads": heads}, _ref(qb, kb, vb, heads, rb.astype(np.float64)))


def test_supported():
    q = torch.zeros(2, 8, 96, device="cuda", dtype=torch.float16)
    declined = [(q.float(), q.float(), q.float(), 3, False), (q.cpu(), q.cpu(), q.cpu(), 3, False),
                (q[..., :80], q[..., :80], q[..., :80], 2, False), (q, q[:, :4], q[:, :4], 3, True)]
    assert A.supported(q, q, q, 3) and A.supported(q, q, q, 3, causal=True)
    for qq, kk, vv, heads, causal in declined:
        assert not A.supported(qq, kk, vv, heads, causal=causal)
        with pytest.raises(ValueError):
            A.attention(qq, kk, vv, heads, causal=causal)
