// Fused epilogue / post-processing kernels of the ONNX executor (module _nn).
// dtype: 0 fp32, 1 fp16, 2 bf16. act: 0 none, 1 relu, 2 leaky(alpha),
// 3 sigmoid, 4 clip(0, alpha). All pointers are device pointers.
#pragma once
#include <cstdint>

namespace smlnn {

bool NnGpuAvailable();
// y = act(x * scale[c] + shift[c] + res); scale/shift/res may be null; y may alias x.
void AffineAct(const void* x, int64_t n, int C, int HW, int nhwc, const float* scale, const float* shift,
               const void* res, int act, float alpha, int dtype, void* y, void* stream);
// sum = a + b; act_out = act(sum * scale[c] + shift[c]) (one pass, two outputs)
void AddAffineAct(const void* a, const void* b, int64_t n, int C, int HW, int nhwc, const float* scale,
                  const float* shift, int act, int dtype, void* sum_out, void* act_out, void* stream);
// NHWC max pool (symmetric pads, -inf padding, no dilation), C % 8 == 0
// shift (per channel, fp32, may be null) and relu: epilogue applied to the pooled maxima
void MaxPoolNhwc(const void* x, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw, int OH,
                 int OW, int dtype, void* y, void* stream, const float* shift = nullptr, int relu = 0);
// NHWC global average pool -> fp32 [N, C]
void GapNhwc(const void* x, int N, int HW, int C, int dtype, void* out, void* stream);  // out: input dtype
// Implicit-GEMM MFMA convolution with fused prologue/epilogue (conv_mfma.hip).
struct ConvArgs {
  const void* x;           // NHWC [B, H, W, C]
  const void* w;           // [Cout][R][S][C]
  void* y;                 // NHWC [B, OH, OW, Cout]
  const float* in_scale;   // prologue affine per input channel (null: none)
  const float* in_shift;
  const float* bias;       // per output channel (null: none)
  const void* res;         // residual, same layout as y (null: none)
  const float* out_scale;  // second output y2 = relu(y * out_scale + out_shift) (null: none)
  const float* out_shift;
  void* y2;
  int B, H, W, C, Cout, R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, OH, OW;
  int relu;            // 0 none, 1 after bias (before the residual add), 2 after the residual add
  int prologue_relu;   // relu after the prologue affine
  int kernel = 0;      // 0 picks the tile by shape; BM*1000+BN forces one (64064, 128064, 64128,
                       // 128128, 256128, 128256)
  // split-K (ConvSplitPlan): split_k > 1 K ranges per output tile, fp32 partial tiles in ws, one arrival
  // counter per tile in ws_cnt (zeroed before the launch); the last arriving split sums and runs the epilogue
  int split_k = 1;
  float* ws = nullptr;
  int* ws_cnt = nullptr;
};
constexpr int kConvStem = 1;  // ConvArgs::kernel: the packed few-channel stem form (C = 4, R = S = 8)
bool ConvMfmaSupported(int C, int Cout, int groups, int dtype);
int ConvMfma(const ConvArgs& a, int dtype, void* stream);
// few-channel (C <= 4) stem conv, K = R * S * C <= 160, weights packed [Cout][160] zero-padded; f16 / bf16
// kp = packed K width: 160 (k = (r * S + s) * C + c) or 192 (C = 3, S * 3 <= 24: k = r * 24 + s * 3 + c)
// form: 0 auto (the row-staged kernel where it applies), 1 the 2-byte gather kernel, 2 row-staged only
int StemConv(const ConvArgs& a, int dtype, void* stream, int kp = 160, int form = 0);
// split-K plan of the tile ConvMfma would pick for a (kernel = 0 only): the number of K splits (1: none) and
// the workspace it needs (fp32 floats, int32 tile counters)
int ConvSplitPlan(const ConvArgs& a, int dtype, int64_t* ws_floats, int* counters);
// K17: batched GEMM with fused epilogue (gemm_mfma.hip), dtype 0 fp32 / 1 fp16 / 2 bf16:
//   C[b] = act(alpha * op(A[b]) * op(B[b]) + beta * (bias[n] | Cin[b]))
// op(A) is [M][K] (trans_a = 0, lda >= K) or A stored [K][M] (trans_a = 1, lda >= M);
// op(B) is [K][N] stored [K][N] (trans_b = 0, ldb >= N) or stored [N][K] (trans_b = 1, ldb >= K).
// Batch strides are in elements (0 = broadcast). Returns 0, or < 0 when the shape is not supported.
struct GemmArgs {
  const void* a = nullptr;
  const void* b = nullptr;
  void* c = nullptr;
  int M = 0, N = 0, K = 0, batch = 1;
  int64_t lda = 0, ldb = 0, ldc = 0;
  int64_t stride_a = 0, stride_b = 0, stride_c = 0;
  int trans_a = 0, trans_b = 0;
  float alpha = 1.f, beta = 1.f;
  const float* bias = nullptr;   // [N] (scaled by beta); batch z reads bias + z * stride_bias
  int64_t stride_bias = 0;
  const void* cmat = nullptr;    // [M][N] additive input, ldcm, batch stride stride_cm (scaled by beta)
  int64_t ldcm = 0, stride_cm = 0;
  int act = 0;                   // 0 none, 1 relu
  // conv = 1: A is the implicit im2col of an NHWC input (any channel count, the 3-channel stem included):
  // row m = (b, oh, ow) of [B, OH, OW], column k = (r, s, c) of [R, S, Cg]; the element is
  // a[((b * H + ih) * W + iw) * C + c] (+ batch stride: a group's channel offset), zero in the padding.
  // K must equal R * S * Cg; M = B * OH * OW; C is the input's pixel stride (all channels).
  int conv = 0;
  int H = 0, W = 0, C = 0, R = 1, S = 1, stride_h = 1, stride_w = 1, pad_h = 0, pad_w = 0, dil_h = 1, dil_w = 1;
  int OH = 0, OW = 0;
};
int GemmMfma(const GemmArgs& g, int dtype, void* stream);
// K18: quantised batched GEMM / implicit-GEMM convolution on the int8 MFMA (qgemm_mfma.hip):
//   acc[m, n] = sum_k (A[m, k] - a_zp[m]) * (B[k, n] - b_zp[n]) (+ bias[n]);  out = acc (int32) or
//   sat(rint(double(acc) * (double(a_scale) * double(b_scale[n])) / double(y_scale)) + y_zp) (u8 / s8).
// A is [M][K] (lda >= K) u8 or s8; B is stored [K][N] (trans_b = 0, ldb >= N) or [N][K] (trans_b = 1).
// Zero points, scales and bias are device pointers read by the kernel (a zero point has its operand's
// type; a *_stride of 0 is a scalar, 1 a vector per row of A / per column of B). Batch strides are in
// elements (0 = broadcast); batch z reads the per-column vectors at z * stride_n. K <= 32768.
// Returns 0, or < 0 when the shape is not supported (-4: K or the batch is out of range).
struct QGemmArgs {
  const void* a = nullptr;
  const void* b = nullptr;
  void* c = nullptr;
  int M = 0, N = 0, K = 0, batch = 1;
  int64_t lda = 0, ldb = 0, ldc = 0;
  int64_t stride_a = 0, stride_b = 0, stride_c = 0;
  int trans_b = 0;
  int a_signed = 0, b_signed = 0;
  int out = 0;                       // 0 int32, 1 u8, 2 s8
  const void* a_zp = nullptr;        // null: 0
  const void* b_zp = nullptr;
  int a_zp_stride = 0, b_zp_stride = 0;
  const float* a_scale = nullptr;    // out != 0: scalar
  const float* b_scale = nullptr;    // scalar or per column
  int b_scale_stride = 0;
  const float* y_scale = nullptr;
  const void* y_zp = nullptr;        // one u8 / s8 (the output type)
  const int32_t* bias = nullptr;     // [N] per batch entry, or null
  int64_t stride_n = 0;
  // conv = 1: A is the implicit im2col of an NHWC u8 / s8 input, as in GemmArgs (trans_b = 1, a_zp scalar:
  // the padding holds the zero point)
  int conv = 0;
  int H = 0, W = 0, C = 0, R = 1, S = 1, stride_h = 1, stride_w = 1, pad_h = 0, pad_w = 0, dil_h = 1, dil_w = 1;
  int OH = 0, OW = 0;
};
int QGemmMfma(const QGemmArgs& g, void* stream);
// K22: fused online-softmax attention forward on the f16 / bf16 MFMA (attn_mfma.hip), dtype 1 fp16 / 2 bf16:
//   out[b, s, h, :] = softmax_l(scale * q[b,s,h,:] . k[b,l,h,:] + key_add[b,l] + bias[b,h,s,l] + causal(s,l))
//                     . v[b,l,h,:]
// q [B, S, heads, d], k / v [B, L, heads, d] are read through element strides (batch, row, head; unit stride
// along d; pointers 16-byte aligned, strides multiples of 8); out is [B, S, heads * d] contiguous in the
// input dtype. d is 32, 64 or 128. causal: key l is visible to query s iff l <= s + (L - S) (needs L >= S).
// Returns 0, or < 0 when the shape is not supported (-4: head size, causal with L < S, B or heads > 65535,
// misaligned operands).
struct AttnArgs {
  const void* q = nullptr;
  const void* k = nullptr;
  const void* v = nullptr;
  void* out = nullptr;
  int B = 0, heads = 0, S = 0, L = 0, d = 0;
  int64_t q_sb = 0, q_sr = 0, q_sh = 0;
  int64_t k_sb = 0, k_sr = 0, k_sh = 0;
  int64_t v_sb = 0, v_sr = 0, v_sh = 0;
  float scale = 1.f;               // applied to the fp32 scores before the additive terms
  const float* key_add = nullptr;  // [B][L] added to every query row, or null
  const float* bias = nullptr;     // element (b, h, s, l) at b * bias_sb + h * bias_sh + s * bias_sr + l, or null
  int64_t bias_sb = 0, bias_sh = 0, bias_sr = 0;  // 0 = broadcast
  int causal = 0;
};
int AttnMfma(const AttnArgs& a, int dtype, void* stream);
// K23: fused top-k maximum-inner-product search on the fp32 MFMA (mips_topk.hip): per query row of q [M, D] the
// k largest q[m, :] . keys[n, :] over keys [N, D], descending, ties by the smaller n; vals fp32 [M, k], idx
// int32 [M, k], slots that cannot be filled hold -inf / -1. Rows have unit stride along D and pitches in
// floats (multiples of 4, readable up to D rounded up to 4; pointers 16-byte aligned). Optional conditioner:
// key_label int32 [N] (dense label ids) and allow uint32 [M, W] (bit l of row m set: label l is eligible for
// query m; a label outside [0, 32 W) is never eligible); both null or both set. splits > 1 spreads the keys
// of a query tile over that many blocks through ws (uint64 [splits][M][k]); 0 takes MipsSplitPlan. Every
// value is read on the device. Returns 0, or < 0 when not supported (-4: k > 64, W > kMipsMaxLabels / 32,
// N > 2^31 - 256, pitches or alignment the 16-byte loads cannot read).
constexpr int kMipsMaxLabels = 2048;
struct MipsArgs {
  const float* q = nullptr;
  const float* keys = nullptr;
  float* vals = nullptr;
  int32_t* idx = nullptr;
  int M = 0, N = 0, D = 0, k = 0;
  int64_t q_pitch = 0, k_pitch = 0;
  const int32_t* key_label = nullptr;
  const uint32_t* allow = nullptr;
  int W = 0;
  int splits = 0;
  uint64_t* ws = nullptr;
};
// key splits the shapes and the CU count suggest (1: the query tiles fill the device on their own)
int MipsSplitPlan(int M, int N, int k, int conditioned);
int MipsTopk(const MipsArgs& a, void* stream);
// K24: fused persistent LSTM / GRU on the fp32 MFMA (rnn_mfma.hip): one launch runs all T steps of every
// direction with the state of a 16-item batch tile on chip. Default activations (Sigmoid, Tanh), fp32.
//   xw   [nd][T][N][gates * Hp]: the input projection with Wb and every part of Rb that is added before an
//        activation (LSTM: all of it; GRU: Rbz, Rbr, and Rbh when linear_before_reset = 0), each gate padded
//        with zeros to Hp = H rounded up to 16. Gates: LSTM i, o, f, c; GRU z, r, h.
//   r    [nd][Hp / 16 unit tiles][gates][Hp / 16 k chunks][64 lanes][4]: value (lane, j) is
//        R[gate * H + 16 tile + lane % 16][16 chunk + 4 (lane / 16) + j], zero past H
//   h0, c0 [nd][N][H] or null (zeros); peep [nd][3][Hp] (i, o, f; zero-padded) or null; rbh [nd][Hp] or null
//   (GRU, linear_before_reset = 1); lens int32 [N] or null (every item runs T steps; values are clamped to
//   [0, T]); y [T][nd][N][H] (every element is written), yh [nd][N][H], yc [nd][N][H] or null.
// Bit d of reverse: direction d walks time backwards from its length. clip 0: none. xw, r, peep, rbh are
// 16-byte aligned, y / yh / yc too when H % 4 == 0. Every value is read on the device. Returns 0, or < 0 when
// not supported (-4: H > 512, nd > 2, an empty dimension, a negative clip, misaligned operands).
struct RnnArgs {
  int cell = 0;  // 0 LSTM, 1 GRU
  const float* xw = nullptr;
  const float* r = nullptr;
  const float* h0 = nullptr;
  const float* c0 = nullptr;
  const float* peep = nullptr;
  const float* rbh = nullptr;
  const int32_t* lens = nullptr;
  float* y = nullptr;
  float* yh = nullptr;
  float* yc = nullptr;
  int T = 0, N = 0, H = 0, nd = 1;
  int reverse = 0;
  float clip = 0.f;
  int linear_before_reset = 0;  // GRU
  int coupled = 0;              // LSTM input_forget: f = 1 - i
};
int RnnMfma(const RnnArgs& a, void* stream);
// K25: fused row normalisation (norm_rows.hip), dtype 0 fp32 / 1 fp16 / 2 bf16 for the activation, the outputs
// and the embedding tables; bias / gamma / beta carry their own dtype code. Per row r of N <= 8192 elements:
//   v = x[r] | x[r] + skip[r % skip_rows] (+ bias[N]) | word[ids[r]] + pos[pos_ids[r]] (+ seg[seg_ids[r]])
//   y[r] = (v - mean) * inv_std * gamma + beta   (rms: mean = 0, inv = rsqrt(mean(v^2) + eps), no beta)
// in fp32 with two-pass statistics. The source is the gather when word is set, the skip form when skip is
// set. x and skip rows have unit inner stride and pitches x_rs / skip_rs in elements; the tables and the
// outputs are contiguous with pitch N. pos_ids null: row r takes position r % S. ids are int32 or int64
// (ids64) and are clamped to their table before use. Optional outputs: sum (v rounded once to the activation
// dtype), mean and inv (fp32 [rows]). 16-byte accesses are used when N and every pointer and pitch allow
// them. Returns 0, or -4 when not supported (N > 8192, empty, inconsistent operands).
struct NormRowsArgs {
  const void* x = nullptr;
  const void* skip = nullptr;
  const void* bias = nullptr;
  const void* gamma = nullptr;
  const void* beta = nullptr;
  void* y = nullptr;
  void* sum = nullptr;
  float* mean = nullptr;
  float* inv = nullptr;
  const void* ids = nullptr;
  const void* pos_ids = nullptr;
  const void* seg_ids = nullptr;
  const void* word = nullptr;
  const void* pos = nullptr;
  const void* seg = nullptr;
  int64_t rows = 0, x_rs = 0, skip_rs = 0, skip_rows = 0;
  int N = 0, rms = 0, ids64 = 0, S = 1, word_rows = 0, pos_rows = 0, seg_rows = 0;
  int bias_dt = 0, gamma_dt = 0, beta_dt = 0;
  float eps = 0.f;
};
int NormRows(const NormRowsArgs& a, int dtype, void* stream);
// y = act(x + bias[N]) over rows of pitch x_rs, y contiguous; bias may be null and has its own dtype code.
// mode 0 erf GELU, 1 tanh GELU, 2 v * sigmoid(alpha * v); fp32 math. Returns 0, or -4 when not supported.
int BiasAct(const void* x, int64_t x_rs, const void* bias, int bias_dt, void* y, int64_t rows, int N, int mode,
            float alpha, int dtype, void* stream);
// K26: fused forest walk for the ai.onnx.ml TreeEnsemble operators (forest_walk.hip; the record layout is
// described there). x is fp32 [n, F] with unit inner stride and row pitch x_rs; nodes are 16-byte records
// (16-byte aligned), list 8-byte (id, weight bits) pairs of the leaves with several entries (may be null when
// there are none), tree_off int32 [T + 1], tree_depth int32 [T], chunk_tree int32 [C + 1]. Scores are the fp32
// sum over the trees of the reached leaves' entries, divided by T (average), plus base [K] (may be null), then
// post 0 none / 1 logistic / 2 softmax. out is fp32 [n, K], or [n, 2] for binary (K = 1: [1 - p, p] under
// logistic, else [-s, s]; label index s > 0). classifier: label int64 [n] gets labels[argmax] (the index when
// labels is null), lowest index on ties. launch 0 picks the launch shape by batch size, 1 forces the
// row-parallel kernel, 2 the tree-parallel one, which needs ws: ForestWalkPlan's slices * n * K floats.
// The caller guarantees what the device arrays hold: feature ids < F, child indices inside their tree, ids
// < K, list ranges inside the list. Returns 0, or -4 when not supported (K > 192, K > 48 tree-parallel, a
// workspace too small, an empty dimension).
constexpr int kForestChunkNodes = 1024;     // nodes of the LDS forest buffer of the row-parallel kernel
constexpr int kForestRegK = 8;              // largest K whose scores are kept in registers
constexpr int kForestRowBlocksPerCu = 1;    // launch 0: row-parallel from this many row tiles per CU on
struct ForestArgs {
  const float* x = nullptr;
  int64_t x_rs = 0, n = 0;
  const void* nodes = nullptr;
  const void* list = nullptr;
  const int32_t* tree_off = nullptr;
  const int32_t* tree_depth = nullptr;
  const int32_t* chunk_tree = nullptr;
  int F = 0, T = 0, C = 0, K = 0;
  const float* base = nullptr;
  int average = 0, post = 0, binary = 0, classifier = 0;
  float* out = nullptr;
  int64_t* label = nullptr;
  const int64_t* labels = nullptr;
  int launch = 0;
  float* ws = nullptr;
  int64_t ws_floats = 0;
};
// the launch shape ForestWalk would take (1 row-parallel, 2 tree-parallel; -4: not supported) and, for the
// tree-parallel one, the number of forest slices of its workspace (0 otherwise)
int ForestWalkPlan(int64_t n, int F, int T, int K, int launch, int* slices);
int ForestWalk(const ForestArgs& a, void* stream);
// K27: one ALS half-sweep (als_mfma.hip): X[row] of every task's row is solved from the factors Y of the other
// side. X [nX, kp] and Y [nY, kp] are fp64 with kp = k padded to a multiple of 16 and zero pad columns, both
// 128-byte aligned. indices int32 / val fp64 are the CSR payload of X's side; tasks int64 [ntasks, 4] are
// (row, first nonzero, length <= seg_len, slot or -1), red int64 [nred, 4] are (row, first slot, slots, n_r) of
// the rows cut into segments (may be null when nred == 0); slots is the number of workspace slots the tasks
// name. ws holds max(slots, implicit ? ceil(nY / seg_len) : 0) * (kp kp + kp) doubles; yty [kp, kp] is written
// and read by an implicit sweep. The caller guarantees what the device arrays hold: indices in [0, nY), rows in
// [0, nX), nonzero ranges inside indices / val, slot ranges inside slots. Returns 0, -3 when a launch fails, or
// -4 when not supported (k outside 1 .. 64, lam not positive and finite, a workspace too small).
constexpr int kAlsMaxRank = 64;
struct AlsArgs {
  const int32_t* indices = nullptr;
  const double* val = nullptr;
  const int64_t* tasks = nullptr;
  const int64_t* red = nullptr;
  const double* Y = nullptr;
  double* X = nullptr;
  double* yty = nullptr;
  double* ws = nullptr;
  int64_t nX = 0, nY = 0, ntasks = 0, nred = 0, slots = 0, ws_doubles = 0;
  int k = 0, kp = 0, seg_len = 0, implicit = 0, nonnegative = 0;
  double lam = 0.0, alpha = 0.0;
};
int AlsSweep(const AlsArgs& a, void* stream);
// Direct grouped / depthwise NHWC convolution (conv_direct.hip): x [B,H,W,C], w [Cout][R][S][C/groups],
// y [B,OH,OW,Cout]; fp32 accumulation; y = conv + bias, relu (1: before the residual add, 2: after), + res.
struct GroupConvArgs {
  const void* x;
  const void* w;
  void* y;
  const float* bias;
  const void* res;
  int B, H, W, C, Cout, R, S, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, OH, OW, groups, relu;
};
int GroupConv(const GroupConvArgs& a, int dtype, void* stream);
// fp32 row softmax (y may be null) and argmax (amax may be null)
void SoftmaxRows(const float* x, int rows, int cols, float* y, int64_t* amax, void* stream);

}  // namespace smlnn
