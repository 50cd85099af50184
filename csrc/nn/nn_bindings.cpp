// pybind11 module _nn: raw-pointer entry points (torch data_ptr + stream).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "nn_ops.h"

namespace py = pybind11;
using namespace smlnn;

template <class T>
static T* P(uintptr_t p) {
  return reinterpret_cast<T*>(p);
}

PYBIND11_MODULE(_nn, m) {
  m.doc() = "MI355X fused epilogue kernels for the ONNX executor";
  m.def("gpu_available", &NnGpuAvailable);
  m.def("affine_act", [](uintptr_t x, int64_t n, int C, int HW, int nhwc, uintptr_t scale, uintptr_t shift,
                         uintptr_t res, int act, float alpha, int dtype, uintptr_t y, uintptr_t stream) {
    AffineAct(P<const void>(x), n, C, HW, nhwc, P<const float>(scale), P<const float>(shift), P<const void>(res), act,
              alpha, dtype, P<void>(y), P<void>(stream));
  });
  m.def("add_affine_act", [](uintptr_t a, uintptr_t b, int64_t n, int C, int HW, int nhwc, uintptr_t scale,
                             uintptr_t shift, int act, int dtype, uintptr_t sum_out, uintptr_t act_out,
                             uintptr_t stream) {
    AddAffineAct(P<const void>(a), P<const void>(b), n, C, HW, nhwc, P<const float>(scale), P<const float>(shift), act,
                 dtype, P<void>(sum_out), P<void>(act_out), P<void>(stream));
  });
  m.def("gap_nhwc", [](uintptr_t x, int N, int HW, int C, int dtype, uintptr_t out, uintptr_t stream) {
    GapNhwc(P<const void>(x), N, HW, C, dtype, P<void>(out), P<void>(stream));
  });
  m.def("maxpool_nhwc", [](uintptr_t x, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                           int OH, int OW, int dtype, uintptr_t y, uintptr_t stream, uintptr_t shift, int relu) {
    MaxPoolNhwc(reinterpret_cast<const void*>(x), N, H, W, C, kh, kw, sh, sw, ph, pw, OH, OW, dtype,
                reinterpret_cast<void*>(y), reinterpret_cast<void*>(stream), reinterpret_cast<const float*>(shift), relu);
  }, pybind11::arg("x"), pybind11::arg("N"), pybind11::arg("H"), pybind11::arg("W"), pybind11::arg("C"),
     pybind11::arg("kh"), pybind11::arg("kw"), pybind11::arg("sh"), pybind11::arg("sw"), pybind11::arg("ph"),
     pybind11::arg("pw"), pybind11::arg("OH"), pybind11::arg("OW"), pybind11::arg("dtype"), pybind11::arg("y"),
     pybind11::arg("stream"), pybind11::arg("shift") = 0, pybind11::arg("relu") = 0);
  m.def("conv_supported", &ConvMfmaSupported);
  m.def("conv_mfma", [](uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t in_scale, uintptr_t in_shift,
                        uintptr_t bias, uintptr_t res, uintptr_t out_scale, uintptr_t out_shift, uintptr_t y2,
                        std::vector<int> g, int relu, int prologue_relu, int dtype, uintptr_t stream, int kernel,
                        int split_k, uintptr_t ws, uintptr_t ws_cnt) {
    if (g.size() != 15) throw std::invalid_argument("geometry: B,H,W,C,Cout,R,S,sh,sw,ph,pw,dh,dw,OH,OW");
    ConvArgs a{P<const void>(x), P<const void>(w), P<void>(y), P<const float>(in_scale), P<const float>(in_shift),
               P<const float>(bias), P<const void>(res), P<const float>(out_scale), P<const float>(out_shift),
               P<void>(y2), g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12], g[13],
               g[14], relu, prologue_relu, kernel, split_k, P<float>(ws), P<int>(ws_cnt)};
    const int rc = ConvMfma(a, dtype, P<void>(stream));
    if (rc != 0) throw std::runtime_error("conv_mfma failed (rc=" + std::to_string(rc) + ")");
  }, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("y"), pybind11::arg("in_scale"), pybind11::arg("in_shift"),
     pybind11::arg("bias"), pybind11::arg("res"), pybind11::arg("out_scale"), pybind11::arg("out_shift"),
     pybind11::arg("y2"), pybind11::arg("geom"), pybind11::arg("relu"), pybind11::arg("prologue_relu"),
     pybind11::arg("dtype"), pybind11::arg("stream"), pybind11::arg("kernel") = 0, pybind11::arg("split_k") = 1,
     pybind11::arg("ws") = 0, pybind11::arg("ws_cnt") = 0);
  // few-channel stem conv: w packed [Cout][160] (ops.conv.pack_stem_weight)
  // (in_scale / in_shift: optional per-input-channel affine (+ ReLU) applied to the im2col values, padding
  // taps stay 0 - the input BatchNormalization of an image model)
  m.def("stem_conv", [](uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t bias, uintptr_t res, std::vector<int> g,
                        int relu, int dtype, uintptr_t stream, uintptr_t in_scale, uintptr_t in_shift, int pro_relu,
                        int kp, int form) {
    if (g.size() != 15) throw std::invalid_argument("geometry: B,H,W,C,Cout,R,S,sh,sw,ph,pw,dh,dw,OH,OW");
    if ((in_scale == 0) != (in_shift == 0)) throw std::invalid_argument("in_scale and in_shift go together");
    ConvArgs a{P<const void>(x), P<const void>(w), P<void>(y), P<const float>(in_scale), P<const float>(in_shift),
               P<const float>(bias), P<const void>(res), nullptr, nullptr, nullptr, g[0], g[1], g[2], g[3], g[4], g[5],
               g[6], g[7], g[8], g[9], g[10], g[11], g[12], g[13], g[14], relu, pro_relu, 0};
    const int rc = StemConv(a, dtype, P<void>(stream), kp, form);
    if (rc != 0) throw std::runtime_error("stem_conv failed (rc=" + std::to_string(rc) + ")");
  }, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("y"), pybind11::arg("bias"), pybind11::arg("res"),
     pybind11::arg("geom"), pybind11::arg("relu"), pybind11::arg("dtype"), pybind11::arg("stream"),
     pybind11::arg("in_scale") = 0, pybind11::arg("in_shift") = 0, pybind11::arg("pro_relu") = 0,
     pybind11::arg("kp") = 160, pybind11::arg("form") = 0);
  // split-K plan of the default tile: (splits, workspace fp32 floats, int32 counters)
  m.def("conv_split_plan", [](std::vector<int> g, int dtype, bool has_prologue, int kernel) {
    if (g.size() != 15) throw std::invalid_argument("geometry: B,H,W,C,Cout,R,S,sh,sw,ph,pw,dh,dw,OH,OW");
    static const float dummy = 0.f;
    ConvArgs a{nullptr, nullptr, nullptr, has_prologue ? &dummy : nullptr, nullptr, nullptr, nullptr, nullptr,
               nullptr, nullptr, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12], g[13],
               g[14], 0, 0, kernel};
    int64_t wsf = 0;
    int cnt = 0;
    const int sk = ConvSplitPlan(a, dtype, &wsf, &cnt);
    return pybind11::make_tuple(sk, wsf, cnt);
  }, pybind11::arg("geom"), pybind11::arg("dtype"), pybind11::arg("has_prologue"), pybind11::arg("kernel") = 0);
  // conv: [] or [H, W, C, R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, OH, OW] (implicit im2col A)
  m.def("gemm", [](uintptr_t a, uintptr_t b, uintptr_t c, int M, int N, int K, int batch, int64_t lda, int64_t ldb,
                   int64_t ldc, int64_t sa, int64_t sb, int64_t sc, int trans_a, int trans_b, float alpha, float beta,
                   uintptr_t bias, uintptr_t cmat, int64_t ldcm, int64_t scm, int act, int dtype, uintptr_t stream,
                   std::vector<int> conv, int64_t stride_bias) {
    GemmArgs g;
    if (!conv.empty()) {
      if (conv.size() != 13) throw std::invalid_argument("conv geometry: H,W,C,R,S,sh,sw,ph,pw,dh,dw,OH,OW");
      g.conv = 1;
      g.H = conv[0]; g.W = conv[1]; g.C = conv[2]; g.R = conv[3]; g.S = conv[4]; g.stride_h = conv[5];
      g.stride_w = conv[6]; g.pad_h = conv[7]; g.pad_w = conv[8]; g.dil_h = conv[9]; g.dil_w = conv[10];
      g.OH = conv[11]; g.OW = conv[12];
    }
    g.stride_bias = stride_bias;
    g.a = P<const void>(a); g.b = P<const void>(b); g.c = P<void>(c);
    g.M = M; g.N = N; g.K = K; g.batch = batch;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.stride_a = sa; g.stride_b = sb; g.stride_c = sc;
    g.trans_a = trans_a; g.trans_b = trans_b; g.alpha = alpha; g.beta = beta;
    g.bias = P<const float>(bias); g.cmat = P<const void>(cmat); g.ldcm = ldcm; g.stride_cm = scm; g.act = act;
    const int rc = GemmMfma(g, dtype, P<void>(stream));
    if (rc != 0) throw std::runtime_error("gemm_mfma failed (rc=" + std::to_string(rc) + ")");
  }, pybind11::arg("a"), pybind11::arg("b"), pybind11::arg("c"), pybind11::arg("M"), pybind11::arg("N"),
     pybind11::arg("K"), pybind11::arg("batch"), pybind11::arg("lda"), pybind11::arg("ldb"), pybind11::arg("ldc"),
     pybind11::arg("sa"), pybind11::arg("sb"), pybind11::arg("sc"), pybind11::arg("trans_a"), pybind11::arg("trans_b"),
     pybind11::arg("alpha"), pybind11::arg("beta"), pybind11::arg("bias"), pybind11::arg("cmat"), pybind11::arg("ldcm"),
     pybind11::arg("scm"), pybind11::arg("act"), pybind11::arg("dtype"), pybind11::arg("stream"),
     pybind11::arg("conv") = std::vector<int>(), pybind11::arg("stride_bias") = 0);
  // quantised GEMM / conv (K18). ptrs: a_zp, b_zp, a_scale, b_scale, y_scale, y_zp, bias (0 = absent);
  // flags: trans_b, a_signed, b_signed, out (0 int32, 1 u8, 2 s8), a_zp_stride, b_zp_stride, b_scale_stride;
  // conv as in gemm. Returns false when the kernel does not take the shape (nothing was launched).
  m.def("qgemm", [](uintptr_t a, uintptr_t b, uintptr_t c, int M, int N, int K, int batch, int64_t lda, int64_t ldb,
                    int64_t ldc, int64_t sa, int64_t sb, int64_t sc, std::vector<int> flags,
                    std::vector<uintptr_t> ptrs, int64_t stride_n, uintptr_t stream, std::vector<int> conv) {
    if (flags.size() != 7 || ptrs.size() != 7) throw std::invalid_argument("qgemm: 7 flags, 7 pointers");
    QGemmArgs g;
    if (!conv.empty()) {
      if (conv.size() != 13) throw std::invalid_argument("conv geometry: H,W,C,R,S,sh,sw,ph,pw,dh,dw,OH,OW");
      g.conv = 1;
      g.H = conv[0]; g.W = conv[1]; g.C = conv[2]; g.R = conv[3]; g.S = conv[4]; g.stride_h = conv[5];
      g.stride_w = conv[6]; g.pad_h = conv[7]; g.pad_w = conv[8]; g.dil_h = conv[9]; g.dil_w = conv[10];
      g.OH = conv[11]; g.OW = conv[12];
    }
    g.a = P<const void>(a); g.b = P<const void>(b); g.c = P<void>(c);
    g.M = M; g.N = N; g.K = K; g.batch = batch;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.stride_a = sa; g.stride_b = sb; g.stride_c = sc;
    g.trans_b = flags[0]; g.a_signed = flags[1]; g.b_signed = flags[2]; g.out = flags[3];
    g.a_zp_stride = flags[4]; g.b_zp_stride = flags[5]; g.b_scale_stride = flags[6];
    g.a_zp = P<const void>(ptrs[0]); g.b_zp = P<const void>(ptrs[1]); g.a_scale = P<const float>(ptrs[2]);
    g.b_scale = P<const float>(ptrs[3]); g.y_scale = P<const float>(ptrs[4]); g.y_zp = P<const void>(ptrs[5]);
    g.bias = P<const int32_t>(ptrs[6]);
    g.stride_n = stride_n;
    const int rc = QGemmMfma(g, P<void>(stream));
    if (rc == -4) return false;
    if (rc != 0) throw std::runtime_error("qgemm_mfma failed (rc=" + std::to_string(rc) + ")");
    return true;
  }, pybind11::arg("a"), pybind11::arg("b"), pybind11::arg("c"), pybind11::arg("M"), pybind11::arg("N"),
     pybind11::arg("K"), pybind11::arg("batch"), pybind11::arg("lda"), pybind11::arg("ldb"), pybind11::arg("ldc"),
     pybind11::arg("sa"), pybind11::arg("sb"), pybind11::arg("sc"), pybind11::arg("flags"), pybind11::arg("ptrs"),
     pybind11::arg("stride_n"), pybind11::arg("stream"), pybind11::arg("conv") = std::vector<int>());
  // fused attention (K22). dims: B, heads, S, L, d, causal; strides (elements): q, k, v (batch, row, head)
  // each, then bias (batch, head, row); key_add / bias: 0 = absent. Returns false when the kernel does not
  // take the shape (nothing was launched).
  m.def("attention", [](uintptr_t q, uintptr_t k, uintptr_t v, uintptr_t out, std::vector<int> dims,
                        std::vector<int64_t> strides, float scale, uintptr_t key_add, uintptr_t bias, int dtype,
                        uintptr_t stream) {
    if (dims.size() != 6 || strides.size() != 12) throw std::invalid_argument("attention: 6 dims, 12 strides");
    AttnArgs a;
    a.q = P<const void>(q); a.k = P<const void>(k); a.v = P<const void>(v); a.out = P<void>(out);
    a.B = dims[0]; a.heads = dims[1]; a.S = dims[2]; a.L = dims[3]; a.d = dims[4]; a.causal = dims[5];
    a.q_sb = strides[0]; a.q_sr = strides[1]; a.q_sh = strides[2];
    a.k_sb = strides[3]; a.k_sr = strides[4]; a.k_sh = strides[5];
    a.v_sb = strides[6]; a.v_sr = strides[7]; a.v_sh = strides[8];
    a.bias_sb = strides[9]; a.bias_sh = strides[10]; a.bias_sr = strides[11];
    a.scale = scale; a.key_add = P<const float>(key_add); a.bias = P<const float>(bias);
    const int rc = AttnMfma(a, dtype, P<void>(stream));
    if (rc == -4) return false;
    if (rc != 0) throw std::runtime_error("attn_mfma failed (rc=" + std::to_string(rc) + ")");
    return true;
  }, pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("out"), pybind11::arg("dims"),
     pybind11::arg("strides"), pybind11::arg("scale"), pybind11::arg("key_add"), pybind11::arg("bias"),
     pybind11::arg("dtype"), pybind11::arg("stream"));
  // fused top-k inner-product search (K23). dims: M, N, D, k, W (allow words per query), splits (0: planned);
  // pitches (floats): q, keys; key_label / allow / ws: 0 = absent (ws: uint64 [splits][M][k], needed when
  // splits != 1). Returns false when the kernel does not take the shape (nothing was launched).
  m.def("mips_topk", [](uintptr_t q, uintptr_t keys, uintptr_t vals, uintptr_t idx, std::vector<int> dims,
                        std::vector<int64_t> pitches, uintptr_t key_label, uintptr_t allow, uintptr_t ws,
                        uintptr_t stream) {
    if (dims.size() != 6 || pitches.size() != 2) throw std::invalid_argument("mips_topk: 6 dims, 2 pitches");
    MipsArgs a;
    a.q = P<const float>(q); a.keys = P<const float>(keys); a.vals = P<float>(vals); a.idx = P<int32_t>(idx);
    a.M = dims[0]; a.N = dims[1]; a.D = dims[2]; a.k = dims[3]; a.W = dims[4]; a.splits = dims[5];
    a.q_pitch = pitches[0]; a.k_pitch = pitches[1];
    a.key_label = P<const int32_t>(key_label); a.allow = P<const uint32_t>(allow); a.ws = P<uint64_t>(ws);
    const int rc = MipsTopk(a, P<void>(stream));
    if (rc == -4) return false;
    if (rc != 0) throw std::runtime_error("mips_topk failed (rc=" + std::to_string(rc) + ")");
    return true;
  }, pybind11::arg("q"), pybind11::arg("keys"), pybind11::arg("vals"), pybind11::arg("idx"), pybind11::arg("dims"),
     pybind11::arg("pitches"), pybind11::arg("key_label"), pybind11::arg("allow"), pybind11::arg("ws"),
     pybind11::arg("stream"));
  m.def("mips_split_plan", &MipsSplitPlan);
  m.attr("MIPS_MAX_LABELS") = kMipsMaxLabels;
  // fused persistent LSTM / GRU (K24). ptrs: xw, r, h0, c0, peep, rbh, lens, y, yh, yc (0 = absent); dims: cell
  // (0 LSTM, 1 GRU), T, N, H, nd, reverse bits, linear_before_reset, coupled. Returns false when the kernel
  // does not take the shape (nothing was launched).
  m.def("rnn", [](std::vector<uintptr_t> ptrs, std::vector<int> dims, float clip, uintptr_t stream) {
    if (ptrs.size() != 10 || dims.size() != 8) throw std::invalid_argument("rnn: 10 pointers, 8 dims");
    RnnArgs a;
    a.xw = P<const float>(ptrs[0]); a.r = P<const float>(ptrs[1]); a.h0 = P<const float>(ptrs[2]);
    a.c0 = P<const float>(ptrs[3]); a.peep = P<const float>(ptrs[4]); a.rbh = P<const float>(ptrs[5]);
    a.lens = P<const int32_t>(ptrs[6]); a.y = P<float>(ptrs[7]); a.yh = P<float>(ptrs[8]); a.yc = P<float>(ptrs[9]);
    a.cell = dims[0]; a.T = dims[1]; a.N = dims[2]; a.H = dims[3]; a.nd = dims[4]; a.reverse = dims[5];
    a.linear_before_reset = dims[6]; a.coupled = dims[7];
    a.clip = clip;
    const int rc = RnnMfma(a, P<void>(stream));
    if (rc == -4) return false;
    if (rc != 0) throw std::runtime_error("rnn_mfma failed (rc=" + std::to_string(rc) + ")");
    return true;
  }, pybind11::arg("ptrs"), pybind11::arg("dims"), pybind11::arg("clip"), pybind11::arg("stream"));
  m.def("group_conv", [](uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t bias, uintptr_t res, std::vector<int> g,
                         int groups, int relu, int dtype, uintptr_t stream) {
    if (g.size() != 15) throw std::invalid_argument("geometry: B,H,W,C,Cout,R,S,sh,sw,ph,pw,dh,dw,OH,OW");
    GroupConvArgs a{P<const void>(x), P<const void>(w), P<void>(y), P<const float>(bias), P<const void>(res),
                    g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12], g[13], g[14],
                    groups, relu};
    const int rc = GroupConv(a, dtype, P<void>(stream));
    if (rc != 0) throw std::runtime_error("group_conv failed (rc=" + std::to_string(rc) + ")");
  });
  // fused row normalisation (K25). ptrs (0 = absent): x, skip, bias, gamma, beta, y, sum, mean, inv, ids,
  // pos_ids, seg_ids, word, pos, seg. dims: rows, N, x row pitch, skip row pitch, skip rows, rms, ids64, S,
  // word / pos / seg table rows, dtype, bias / gamma / beta dtype. Returns false when the kernel does not take
  // the problem (nothing was launched).
  m.def("norm_rows", [](std::vector<uintptr_t> ptrs, std::vector<int64_t> dims, float eps, uintptr_t stream) {
    if (ptrs.size() != 15 || dims.size() != 15) throw std::invalid_argument("norm_rows: 15 ptrs, 15 dims");
    NormRowsArgs a;
    a.x = P<const void>(ptrs[0]); a.skip = P<const void>(ptrs[1]); a.bias = P<const void>(ptrs[2]);
    a.gamma = P<const void>(ptrs[3]); a.beta = P<const void>(ptrs[4]); a.y = P<void>(ptrs[5]);
    a.sum = P<void>(ptrs[6]); a.mean = P<float>(ptrs[7]); a.inv = P<float>(ptrs[8]);
    a.ids = P<const void>(ptrs[9]); a.pos_ids = P<const void>(ptrs[10]); a.seg_ids = P<const void>(ptrs[11]);
    a.word = P<const void>(ptrs[12]); a.pos = P<const void>(ptrs[13]); a.seg = P<const void>(ptrs[14]);
    for (size_t i = 4; i < dims.size(); ++i)
      if (dims[i] < 0 || dims[i] > INT32_MAX) return false;
    a.rows = dims[0]; a.N = static_cast<int>(std::min<int64_t>(dims[1], INT32_MAX));
    a.x_rs = dims[2]; a.skip_rs = dims[3]; a.skip_rows = dims[4];
    a.rms = static_cast<int>(dims[5]); a.ids64 = static_cast<int>(dims[6]); a.S = static_cast<int>(dims[7]);
    a.word_rows = static_cast<int>(dims[8]); a.pos_rows = static_cast<int>(dims[9]);
    a.seg_rows = static_cast<int>(dims[10]);
    a.bias_dt = static_cast<int>(dims[12]); a.gamma_dt = static_cast<int>(dims[13]);
    a.beta_dt = static_cast<int>(dims[14]); a.eps = eps;
    const int rc = NormRows(a, static_cast<int>(dims[11]), P<void>(stream));
    if (rc == -4) return false;
    if (rc != 0) throw std::runtime_error("norm_rows failed (rc=" + std::to_string(rc) + ")");
    return true;
  }, pybind11::arg("ptrs"), pybind11::arg("dims"), pybind11::arg("eps"), pybind11::arg("stream"));
  // y = act(x + bias) (K25). dims: rows, N, x row pitch, mode, dtype, bias dtype
  m.def("bias_act", [](uintptr_t x, uintptr_t bias, uintptr_t y, std::vector<int64_t> dims, float alpha,
                       uintptr_t stream) {
    if (dims.size() != 6) throw std::invalid_argument("bias_act: 6 dims");
    if (dims[1] > INT32_MAX) return false;
    const int rc = BiasAct(P<const void>(x), dims[2], P<const void>(bias), static_cast<int>(dims[5]), P<void>(y),
                           dims[0], static_cast<int>(dims[1]), static_cast<int>(dims[3]), alpha,
                           static_cast<int>(dims[4]), P<void>(stream));
    if (rc == -4) return false;
    if (rc != 0) throw std::runtime_error("bias_act failed (rc=" + std::to_string(rc) + ")");
    return true;
  }, pybind11::arg("x"), pybind11::arg("bias"), pybind11::arg("y"), pybind11::arg("dims"), pybind11::arg("alpha"),
     pybind11::arg("stream"));
  // fused forest walk (K26). ptrs (0 = absent): x, nodes, list, tree_off, tree_depth, chunk_tree, base, out,
  // label, labels, ws. dims: n, F, x row pitch, T, C, K, average, post, binary, classifier, launch, ws floats.
  // Returns false when the kernel does not take the problem (nothing was launched).
  m.def("forest_walk", [](std::vector<uintptr_t> ptrs, std::vector<int64_t> dims, uintptr_t stream) {
    if (ptrs.size() != 11 || dims.size() != 12) throw std::invalid_argument("forest_walk: 11 ptrs, 12 dims");
    for (size_t i : {1, 3, 4, 5, 6, 7, 8, 9, 10})
      if (dims[i] < 0 || dims[i] > INT32_MAX) return false;
    ForestArgs a;
    a.x = P<const float>(ptrs[0]); a.nodes = P<const void>(ptrs[1]); a.list = P<const void>(ptrs[2]);
    a.tree_off = P<const int32_t>(ptrs[3]); a.tree_depth = P<const int32_t>(ptrs[4]);
    a.chunk_tree = P<const int32_t>(ptrs[5]); a.base = P<const float>(ptrs[6]); a.out = P<float>(ptrs[7]);
    a.label = P<int64_t>(ptrs[8]); a.labels = P<const int64_t>(ptrs[9]); a.ws = P<float>(ptrs[10]);
    a.n = dims[0]; a.F = static_cast<int>(dims[1]); a.x_rs = dims[2]; a.T = static_cast<int>(dims[3]);
    a.C = static_cast<int>(dims[4]); a.K = static_cast<int>(dims[5]); a.average = static_cast<int>(dims[6]);
    a.post = static_cast<int>(dims[7]); a.binary = static_cast<int>(dims[8]);
    a.classifier = static_cast<int>(dims[9]); a.launch = static_cast<int>(dims[10]); a.ws_floats = dims[11];
    const int rc = ForestWalk(a, P<void>(stream));
    if (rc == -4) return false;
    if (rc != 0) throw std::runtime_error("forest_walk failed (rc=" + std::to_string(rc) + ")");
    return true;
  }, pybind11::arg("ptrs"), pybind11::arg("dims"), pybind11::arg("stream"));
  // (launch shape 1 row-parallel / 2 tree-parallel, workspace slices) of forest_walk; shape -4: not supported
  m.def("forest_plan", [](int64_t n, int64_t F, int64_t T, int64_t K, int launch) {
    int slices = 0;
    if (F > INT32_MAX || T > INT32_MAX || K > INT32_MAX) return std::make_pair(-4, 0);
    const int shape = ForestWalkPlan(n, static_cast<int>(F), static_cast<int>(T), static_cast<int>(K), launch, &slices);
    return std::make_pair(shape, slices);
  });
  // one ALS half-sweep (K27). ptrs (0 = absent): indices, val, tasks, red, Y, X, yty, ws. dims: nX, nY, k, kp,
  // ntasks, nred, slots, ws doubles, seg_len, implicit, nonnegative. scalars: lam, alpha. Returns false when the
  // kernel does not take the problem (nothing was launched).
  m.def("als_sweep", [](std::vector<uintptr_t> ptrs, std::vector<int64_t> dims, std::vector<double> scalars,
                        uintptr_t stream) {
    if (ptrs.size() != 8 || dims.size() != 11 || scalars.size() != 2)
      throw std::invalid_argument("als_sweep: 8 ptrs, 11 dims, 2 scalars");
    for (size_t i : {2, 3, 8, 9, 10})
      if (dims[i] < 0 || dims[i] > INT32_MAX) return false;
    if (ptrs[4] % 128 || ptrs[5] % 128) return false;
    AlsArgs a;
    a.indices = P<const int32_t>(ptrs[0]); a.val = P<const double>(ptrs[1]); a.tasks = P<const int64_t>(ptrs[2]);
    a.red = P<const int64_t>(ptrs[3]); a.Y = P<const double>(ptrs[4]); a.X = P<double>(ptrs[5]);
    a.yty = P<double>(ptrs[6]); a.ws = P<double>(ptrs[7]);
    a.nX = dims[0]; a.nY = dims[1]; a.k = static_cast<int>(dims[2]); a.kp = static_cast<int>(dims[3]);
    a.ntasks = dims[4]; a.nred = dims[5]; a.slots = dims[6]; a.ws_doubles = dims[7];
    a.seg_len = static_cast<int>(dims[8]); a.implicit = static_cast<int>(dims[9]);
    a.nonnegative = static_cast<int>(dims[10]); a.lam = scalars[0]; a.alpha = scalars[1];
    const int rc = AlsSweep(a, P<void>(stream));
    if (rc == -4) return false;
    if (rc != 0) throw std::runtime_error("als_sweep failed (rc=" + std::to_string(rc) + ")");
    return true;
  }, pybind11::arg("ptrs"), pybind11::arg("dims"), pybind11::arg("scalars"), pybind11::arg("stream"));
  m.def("softmax_rows", [](uintptr_t x, int rows, int cols, uintptr_t y, uintptr_t amax, uintptr_t stream) {
    SoftmaxRows(P<const float>(x), rows, cols, P<float>(y), P<int64_t>(amax), P<void>(stream));
  });
}
