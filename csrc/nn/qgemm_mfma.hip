// K18: quantised (u8 / s8) batched GEMM and implicit-GEMM convolution on the CDNA4 int8 matrix cores
// (module _nn; ONNX MatMulInteger / ConvInteger / QLinearMatMul / QLinearConv of the executor).
//
//   acc[m, n] = sum_k (A[m, k] - a_zp[m]) * (B[k, n] - b_zp[n])  (+ bias[n], int32)
//   out = acc                                                                         (int32)
//   out = sat(rint(double(acc) * (double(a_s) * double(b_s[n])) / double(y_s)) + y_zp)  (u8 / s8)
//
// v_mfma_i32_16x16x64_i8 is signed x signed with exact int32 accumulation. A u8 operand becomes s8 at the
// LDS write (XOR 0x80 on whole dwords), its zero point zp - 128. The MFMAs run on the raw shifted bytes;
// the zero points are folded in afterwards from row / column byte sums, which each thread accumulates
// with dot4 against 0x01010101 over the chunks it stages (a thread stages the same rows in every K tile)
// and which meet in LDS after the K loop. The epilogue forms, in int64,
//   S - a_zp'[m] * colsum[n] - b_zp'[n] * rowsum[m] + K * a_zp'[m] * b_zp'[n] + bias[n].
// Bytes past K are staged as shifted zero, so they add nothing to S or to the sums. Zero points, scales
// and bias are read through device pointers here; the launch path reads no tensor value.
//
// Tiling: 256 threads = 4 waves in 2x2, block tile 64 x 64 x 128 bytes of K (two 16x16x64 steps), wave
// tile 32 x 32. The LDS image is double-buffered at a 160-byte row pitch (conflict-free for the 16-lane
// ds_read_b128 fragment reads: a lane's fragment is 16 consecutive k bytes of one row); the next tile's
// global loads are issued before the current tile's MFMAs. The weights (N side) are the MFMA's first
// operand and the rows / pixels (M side) its second, so a lane ends with 4 consecutive n of one m: one
// 16-byte store (int32) or one packed dword (u8 / s8). Staging per operand (template kMode):
//   kVec      K-contiguous rows, 16-B aligned: 16-B buffer loads
//   kBytes    any strides, bytewise, bounds-checked
//   kTrans    B stored [K][N]: a dword (4 n) for each of 4 consecutive k, the 4x4 bytes transposed in
//             registers with v_perm_b32, k-contiguous dwords written
//   kConv     A only: implicit im2col of an NHWC input, k = (r, s, c); padded taps hold the raw x_zp byte
//             (they contribute exactly zero and the row sums stay consistent)
//   kConvVec  kConv with C / groups % 16 == 0: a chunk is 16 channels of one tap, one 16-B load
// Blocks are remapped so each XCD owns a contiguous run of (m, n) tiles.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nn_ops.h"

namespace smlnn {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kBM = 64, kBN = 64, kBK = 128;
constexpr int kLD = 160;  // LDS row pitch in bytes
constexpr int kOnes = 0x01010101;
constexpr int kMaxK = 32768;  // 255 * 255 * K < 2^31: every true accumulator fits in int32

enum { kVec = 0, kBytes = 1, kTrans = 2, kConv = 3, kConvVec = 4 };

struct QLaunch {
  QGemmArgs g;
  int vec_out;  // the 4-n group of a lane may be stored as one 16-B (int32) / 4-B (u8, s8) word
};

// One operand's 64 x 128-byte tile: rows r (m for A, n for B) x k; element (r, k) at base[r * sr + k * sk].
// kVec / kBytes / kConv*: chunk q = tid + 256 i is row q / 8, 16-B chunk q % 8. kTrans: block q is rows
// 4 (q % 16) .. + 3, k = 4 (q / 16) .. + 3.
template <int kMode>
struct QOperand {
  static constexpr int kSums = kMode == kTrans ? 4 : 2;
  const uint8_t* base;
  int64_t sr, sk;
  int rows, K;
  uint32_t flip;  // 0x80808080 for a u8 operand: raw -> shifted s8 bytes
  __amdgpu_buffer_rsrc_t rsrc;
  int sum[kSums];  // byte sums of the shifted rows this thread stages
  // conv gather: this thread's two pixels
  bool row_ok[2];
  int pix[2], ih0[2], iw0[2];
  int H, W, C, S, Cg, dh, dw;
  uint32_t zfill;  // raw x_zp byte x 4

  struct Regs {
    uint32_t d[8];
  };

  __device__ void Init(const void* b, int64_t sr_, int64_t sk_, int rows_, int K_, int is_signed) {
    base = static_cast<const uint8_t*>(b); sr = sr_; sk = sk_; rows = rows_; K = K_;
    flip = is_signed ? 0u : 0x80808080u;
#pragma unroll
    for (int i = 0; i < kSums; ++i) sum[i] = 0;
    if constexpr (kMode == kVec) {
      const int64_t bytes = static_cast<int64_t>(rows - 1) * sr + K;
      rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0, static_cast<int>(bytes), 0x00020000);
    }
  }

  __device__ void InitConv(const QGemmArgs& g, int r0, int tid) {
    H = g.H; W = g.W; C = g.C; S = g.S; dh = g.dil_h; dw = g.dil_w;
    Cg = K / (g.R * g.S);
    const uint32_t z = g.a_zp ? static_cast<const uint8_t*>(g.a_zp)[0] : 0u;
    zfill = z * 0x01010101u;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = r0 + (tid >> 3) + 32 * i;
      row_ok[i] = m < rows;
      pix[i] = 0; ih0[i] = 0; iw0[i] = 0;
      if (row_ok[i]) {
        const int ow = m % g.OW, t = m / g.OW;
        const int oh = t % g.OH, b = t / g.OH;
        ih0[i] = oh * g.stride_h - g.pad_h;
        iw0[i] = ow * g.stride_w - g.pad_w;
        pix[i] = ((b * H + ih0[i]) * W + iw0[i]) * C;  // may be negative: only read with valid taps
      }
    }
  }

  __device__ __forceinline__ void Load(Regs& rg, int r0, int k0, int tid) const {
    if constexpr (kMode == kVec) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int q = tid + kThreads * i;
        const int r = r0 + (q >> 3), k = k0 + (q & 7) * 16;
        const bool ok = r < rows && k < K;
        const uint32_t off = ok ? static_cast<uint32_t>(r * sr + k) : 0x80000000u;
        auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
        uint32_t w[4];
        __builtin_memcpy(w, &v, 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) rg.d[4 * i + j] = ok ? w[j] : flip;
      }
    } else if constexpr (kMode == kBytes) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int q = tid + kThreads * i;
        const int r = r0 + (q >> 3), k = k0 + (q & 7) * 16;
        const uint8_t* p = base + r * sr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t w = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kk = k + 4 * j + e;
            const uint32_t byte = (r < rows && kk < K) ? p[kk * sk] : (flip & 0xffu);
            w |= byte << (8 * e);
          }
          rg.d[4 * i + j] = w;
        }
      }
    } else if constexpr (kMode == kTrans) {
      const int n = r0 + 4 * (tid & 15);  // rows % 4 == 0: n < rows covers n + 3
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + 4 * ((tid >> 4) + 16 * i) + j;
          rg.d[4 * i + j] = (n < rows && k < K) ? *reinterpret_cast<const uint32_t*>(base + k * sk + n) : flip;
        }
    } else {
      // both pixels walk the same k = k0 + 16 (tid % 8) .. + 15 as (tap r, s, channel c)
      const int k = k0 + (tid & 7) * 16;
      int c = k % Cg, t = k / Cg;
      int s = t % S, r = t / S;
      if constexpr (kMode == kConvVec) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int ih = ih0[i] + r * dh, iw = iw0[i] + s * dw;
          const bool in = row_ok[i] && k < K;
          const bool ok = in && ih >= 0 && ih < H && iw >= 0 && iw < W;
          uint4 v = make_uint4(0, 0, 0, 0);
          if (ok) v = *reinterpret_cast<const uint4*>(base + pix[i] + (r * dh * W + s * dw) * C + c);
          const uint32_t fill = in ? zfill : flip;
          rg.d[4 * i + 0] = ok ? v.x : fill;
          rg.d[4 * i + 1] = ok ? v.y : fill;
          rg.d[4 * i + 2] = ok ? v.z : fill;
          rg.d[4 * i + 3] = ok ? v.w : fill;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) rg.d[j] = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int ih = ih0[i] + r * dh, iw = iw0[i] + s * dw;
            const bool in = row_ok[i] && k + e < K;
            const bool ok = in && ih >= 0 && ih < H && iw >= 0 && iw < W;
            uint32_t byte = (in ? zfill : flip) & 0xffu;
            if (ok) byte = base[pix[i] + (r * dh * W + s * dw) * C + c];
            rg.d[4 * i + (e >> 2)] |= byte << (8 * (e & 3));
          }
          if (++c == Cg) {
            c = 0;
            if (++s == S) { s = 0; ++r; }
          }
        }
      }
    }
  }

  __device__ __forceinline__ void Store(const Regs& rg, uint8_t* lds, int tid) {
    if constexpr (kMode == kTrans) {
      const int ng = tid & 15;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int kg = (tid >> 4) + 16 * i;
        const uint32_t d0 = rg.d[4 * i], d1 = rg.d[4 * i + 1], d2 = rg.d[4 * i + 2], d3 = rg.d[4 * i + 3];
        // 4x4 byte transpose: d_k holds n0..n3 of one k; o_n holds k0..k3 of one n
        const uint32_t t0 = __builtin_amdgcn_perm(d1, d0, 0x05010400u), t1 = __builtin_amdgcn_perm(d1, d0, 0x07030602u);
        const uint32_t t2 = __builtin_amdgcn_perm(d3, d2, 0x05010400u), t3 = __builtin_amdgcn_perm(d3, d2, 0x07030602u);
        const uint32_t o[4] = {__builtin_amdgcn_perm(t2, t0, 0x05040100u), __builtin_amdgcn_perm(t2, t0, 0x07060302u),
                               __builtin_amdgcn_perm(t3, t1, 0x05040100u), __builtin_amdgcn_perm(t3, t1, 0x07060302u)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t v = o[j] ^ flip;
          sum[j] = __builtin_amdgcn_sdot4(static_cast<int>(v), kOnes, sum[j], false);
          *reinterpret_cast<uint32_t*>(lds + (4 * ng + j) * kLD + 4 * kg) = v;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int q = tid + kThreads * i;
        uint4 v = make_uint4(rg.d[4 * i] ^ flip, rg.d[4 * i + 1] ^ flip, rg.d[4 * i + 2] ^ flip, rg.d[4 * i + 3] ^ flip);
        int s = sum[i];
        s = __builtin_amdgcn_sdot4(static_cast<int>(v.x), kOnes, s, false);
        s = __builtin_amdgcn_sdot4(static_cast<int>(v.y), kOnes, s, false);
        s = __builtin_amdgcn_sdot4(static_cast<int>(v.z), kOnes, s, false);
        s = __builtin_amdgcn_sdot4(static_cast<int>(v.w), kOnes, s, false);
        sum[i] = s;
        *reinterpret_cast<uint4*>(lds + (q >> 3) * kLD + (q & 7) * 16) = v;
      }
    }
  }

  // add this thread's partial sums into sums[64] (LDS, one entry per tile row)
  __device__ __forceinline__ void Reduce(int* sums, int tid) const {
    if constexpr (kMode == kTrans) {
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(&sums[4 * (tid & 15) + j], sum[j]);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) atomicAdd(&sums[(tid >> 3) + 32 * i], sum[i]);
    }
  }
};

// zero point in the shifted domain (u8: zp - 128); p == nullptr is zero point 0
__device__ __forceinline__ int64_t ShiftedZp(const void* p, int64_t idx, int is_signed) {
  if (is_signed) return p ? static_cast<const int8_t*>(p)[idx] : 0;
  return (p ? static_cast<int>(static_cast<const uint8_t*>(p)[idx]) : 0) - 128;
}

// the host reference's order: (acc * mult) / y_scale, round half to even, + y_zp, saturate
__device__ __forceinline__ int Requant(int64_t acc, double mult, double ys, double yz, double lo, double hi) {
#pragma clang fp contract(off)
  const double p = static_cast<double>(acc) * mult;
  const double q = rint(p / ys) + yz;
  return static_cast<int>(fmin(fmax(q, lo), hi));
}

template <int kAM, int kBMd>
__global__ __launch_bounds__(kThreads) void qgemm_mfma_kernel(QLaunch L) {
  const QGemmArgs& g = L.g;
  constexpr int WM = kBM / 2, WN = kBN / 2, TM = WM / 16, TN = WN / 16;
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * (kBM + kBN) * kLD];
  __shared__ int sums[kBM + kBN];
  uint8_t* As = lds;
  uint8_t* Bs = lds + 2 * kBM * kLD;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tiles_n = (g.N + kBN - 1) / kBN, tiles_m = (g.M + kBM - 1) / kBM;
  const int total = tiles_m * tiles_n;
  int bid = blockIdx.x;
  if ((total & 7) == 0) bid = (bid & 7) * (total >> 3) + (bid >> 3);  // XCD-contiguous tile runs
  const int tn = bid % tiles_n, tm = bid / tiles_n;
  const int m0 = tm * kBM, n0 = tn * kBN;
  const int bz = blockIdx.z;
  if (tid < kBM + kBN) sums[tid] = 0;

  QOperand<kAM> A;
  QOperand<kBMd> B;
  A.Init(static_cast<const uint8_t*>(g.a) + bz * g.stride_a, g.lda, 1, g.M, g.K, g.a_signed);
  if constexpr (kAM == kConv || kAM == kConvVec) A.InitConv(g, m0, tid);
  if (g.trans_b) B.Init(static_cast<const uint8_t*>(g.b) + bz * g.stride_b, g.ldb, 1, g.N, g.K, g.b_signed);
  else B.Init(static_cast<const uint8_t*>(g.b) + bz * g.stride_b, 1, g.ldb, g.N, g.K, g.b_signed);

  v4i acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = v4i{0, 0, 0, 0};
  const int wm0 = (wid >> 1) * WM, wn0 = (wid & 1) * WN;
  const int fr = lane & 15, fg = lane >> 4;
  const int nk = (g.K + kBK - 1) / kBK;

  auto compute = [&](int buf) {
#pragma unroll
    for (int ks = 0; ks < kBK / 64; ++ks) {
      v4i af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        af[i] = *reinterpret_cast<const v4i*>(As + (buf * kBM + wm0 + i * 16 + fr) * kLD + ks * 64 + fg * 16);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bf[j] = *reinterpret_cast<const v4i*>(Bs + (buf * kBN + wn0 + j * 16 + fr) * kLD + ks * 64 + fg * 16);
      // weights first: D[n][m], a lane holds n = 4 (lane / 16) + 0..3 of m = lane % 16
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bf[j], af[i], acc[i][j], 0, 0, 0);
    }
  };

  typename QOperand<kAM>::Regs ra;
  typename QOperand<kBMd>::Regs rb;
  A.Load(ra, m0, 0, tid);
  B.Load(rb, n0, 0, tid);
  A.Store(ra, As, tid);
  B.Store(rb, Bs, tid);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) {
      A.Load(ra, m0, (kt + 1) * kBK, tid);
      B.Load(rb, n0, (kt + 1) * kBK, tid);
    }
    compute(buf);
    if (kt + 1 < nk) {
      A.Store(ra, As + (buf ^ 1) * kBM * kLD, tid);
      B.Store(rb, Bs + (buf ^ 1) * kBN * kLD, tid);
    }
    __syncthreads();
  }
  A.Reduce(sums, tid);
  B.Reduce(sums + kBM, tid);
  __syncthreads();

  // epilogue: lane holds n = n0 + wn0 + 16 j + 4 (lane / 16) + 0..3 of row m = m0 + wm0 + 16 i + lane % 16
  const int64_t nv = bz * g.stride_n;  // this batch entry's offset into the per-column vectors
  const double a_s = g.out ? static_cast<double>(g.a_scale[0]) : 0.0;
  const double y_s = g.out ? static_cast<double>(g.y_scale[0]) : 1.0;
  const double y_z = g.out == 1   ? static_cast<double>(static_cast<const uint8_t*>(g.y_zp)[0])
                     : g.out == 2 ? static_cast<double>(static_cast<const int8_t*>(g.y_zp)[0])
                                  : 0.0;
  const double lo = g.out == 1 ? 0.0 : -128.0, hi = g.out == 1 ? 255.0 : 127.0;
  int64_t rs[TM], az[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int ml = wm0 + i * 16 + fr, m = m0 + ml < g.M ? m0 + ml : g.M - 1;
    rs[i] = sums[ml];
    az[i] = ShiftedZp(g.a_zp, static_cast<int64_t>(m) * g.a_zp_stride, g.a_signed);
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nl = wn0 + j * 16 + 4 * fg, nb = n0 + nl;
    if (nb >= g.N) continue;
    // per column, once for both rows: b_zp', K * b_zp' - colsum (+ bias apart: it is not scaled by a_zp'), scale
    int64_t bzp[4], kc[4], bias[4];
    double mult[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = nb + r < g.N ? nb + r : g.N - 1;
      bzp[r] = ShiftedZp(g.b_zp, (nv + n) * g.b_zp_stride, g.b_signed);
      kc[r] = static_cast<int64_t>(g.K) * bzp[r] - sums[kBM + nl + r];
      bias[r] = g.bias ? g.bias[nv + n] : 0;
      mult[r] = g.out ? a_s * static_cast<double>(g.b_scale[(nv + n) * g.b_scale_stride]) : 0.0;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm0 + i * 16 + fr;
      if (m >= g.M) continue;
      int o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // S - a_zp' colsum - b_zp' rowsum + K a_zp' b_zp' + bias
        const int64_t v = static_cast<int64_t>(acc[i][j][r]) + az[i] * kc[r] - bzp[r] * rs[i] + bias[r];
        o[r] = g.out == 0 ? static_cast<int>(v) : Requant(v, mult[r], y_s, y_z, lo, hi);
      }
      const int64_t at = bz * g.stride_c + static_cast<int64_t>(m) * g.ldc + nb;
      if (g.out == 0) {
        int* c = static_cast<int*>(g.c) + at;
        if (L.vec_out && nb + 3 < g.N) {
          *reinterpret_cast<int4*>(c) = make_int4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (nb + r < g.N) c[r] = o[r];
        }
      } else {
        uint8_t* c = static_cast<uint8_t*>(g.c) + at;
        if (L.vec_out && nb + 3 < g.N) {
          *reinterpret_cast<uint32_t*>(c) = (o[0] & 0xffu) | ((o[1] & 0xffu) << 8) | ((o[2] & 0xffu) << 16) |
                                            (static_cast<uint32_t>(o[3]) << 24);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (nb + r < g.N) c[r] = static_cast<uint8_t>(o[r]);
        }
      }
    }
  }
}

bool Aligned(const void* p, int a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

}  // namespace

int QGemmMfma(const QGemmArgs& g, void* stream) {
  if (g.M <= 0 || g.N <= 0 || g.batch <= 0) return 0;
  if (g.K <= 0 || g.out < 0 || g.out > 2) return -2;
  if (g.K > kMaxK || g.batch > 65535) return -4;  // not supported: the caller keeps its own path
  if (g.out != 0 && (!g.a_scale || !g.b_scale || !g.y_scale || !g.y_zp)) return -2;
  if (static_cast<int64_t>(g.M) * g.ldc >= (1ll << 31) ||
      static_cast<int64_t>(g.trans_b ? g.N : g.K) * g.ldb >= (1ll << 31))
    return -5;  // 32-bit indexing inside one batch entry
  if (g.conv) {
    if (g.R <= 0 || g.S <= 0 || g.K % (g.R * g.S) != 0 || g.OH <= 0 || g.OW <= 0 || g.trans_b != 1 ||
        g.M % (g.OH * g.OW) != 0)
      return -2;
    if (static_cast<int64_t>(g.M / (g.OH * g.OW)) * g.H * g.W * g.C >= (1ll << 31)) return -5;
  } else if (static_cast<int64_t>(g.M) * g.lda >= (1ll << 31)) {
    return -5;
  }
  // K-contiguous rows take 16-B buffer loads when every row start and K are 16-B multiples
  auto vec_ok = [&](const void* p, int64_t ld, int64_t stride, int rows) {
    return Aligned(p, 16) && ld % 16 == 0 && g.K % 16 == 0 && stride % 16 == 0 &&
           static_cast<int64_t>(rows) * ld + g.K < (1ll << 31);
  };
  const int cg = g.conv ? g.K / (g.R * g.S) : 0;
  const int am = g.conv ? (Aligned(g.a, 16) && g.C % 16 == 0 && cg % 16 == 0 && g.stride_a % 16 == 0 ? kConvVec : kConv)
                        : (vec_ok(g.a, g.lda, g.stride_a, g.M) ? kVec : kBytes);
  const int bm = g.trans_b ? (vec_ok(g.b, g.ldb, g.stride_b, g.N) ? kVec : kBytes)
                           : (Aligned(g.b, 4) && g.ldb % 4 == 0 && g.N % 4 == 0 && g.stride_b % 4 == 0 ? kTrans : kBytes);
  QLaunch L;
  L.g = g;
  L.vec_out = Aligned(g.c, g.out == 0 ? 16 : 4) && g.ldc % 4 == 0 && g.stride_c % 4 == 0;
  const int tiles = ((g.M + kBM - 1) / kBM) * ((g.N + kBN - 1) / kBN);
  const dim3 grid(tiles, 1, g.batch);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = -1;
#define SML_QGEMM_CASE(X, Y) \
  if (am == X && bm == Y) { hipLaunchKernelGGL((qgemm_mfma_kernel<X, Y>), grid, dim3(kThreads), 0, st, L); rc = 0; }
  SML_QGEMM_CASE(kVec, kVec) SML_QGEMM_CASE(kVec, kBytes) SML_QGEMM_CASE(kVec, kTrans)
  SML_QGEMM_CASE(kBytes, kVec) SML_QGEMM_CASE(kBytes, kBytes) SML_QGEMM_CASE(kBytes, kTrans)
  SML_QGEMM_CASE(kConv, kVec) SML_QGEMM_CASE(kConv, kBytes)
  SML_QGEMM_CASE(kConvVec, kVec) SML_QGEMM_CASE(kConvVec, kBytes)
#undef SML_QGEMM_CASE
  if (rc != 0) return rc;
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace smlnn
