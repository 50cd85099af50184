// K25: fused row normalisation (LayerNorm / RMSNorm with skip, bias and embedding-gather row sources) and
// bias + GELU kernels for the transformer ops of the ONNX executor on gfx950.
//
// Row kernel. A row of N <= 8192 elements is read once, converted to fp32 and kept in registers until it is
// written: N <= 1024 gives a row to one wave (four rows per 256-thread block, no LDS, no barrier; gamma, beta
// and bias sit in registers for every row the wave visits), larger N gives it to the whole block (wave
// reductions, then a four-entry LDS exchange). Statistics are two-pass from the registers: the mean first,
// then sum((v - mean)^2) over the lanes that hold an element; both sums go through an xor butterfly (DPP
// within a row of 16 lanes, shuffles across), so every lane ends with the same bits. The vector form moves
// 16 bytes per access (8 fp16 / bf16 or 4 fp32 elements) and needs N a multiple of that and every base and
// row pitch 16-byte aligned; the element form has the same structure with lane-interleaved columns and a
// masked tail. gamma / beta / bias carry their own dtype and are converted on load.
//
// Gather source (EmbedLayerNormalization): every id is clamped to [0, table rows - 1] before it is used, so
// an id out of range reads a wrong row instead of faulting (torch raises there).
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "nn_ops.h"

#define NR_HIP_CHECK(e)                                                                                \
  do {                                                                                                 \
    hipError_t _e = (e);                                                                               \
    if (_e != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e)); \
  } while (0)

namespace smlnn {
namespace {

constexpr int kThreads = 256;
constexpr int kWaveMaxN = 1024;
constexpr int kBlockMaxN = 8192;

// ---------------------------------------------------------------- loads / stores by dtype code (0 fp32, 1 fp16, 2 bf16)
__device__ __forceinline__ float lde(const void* p, int dt, int64_t i) {
  if (dt == 0) return static_cast<const float*>(p)[i];
  if (dt == 1) return __half2float(static_cast<const __half*>(p)[i]);
  return __bfloat162float(static_cast<const __hip_bfloat16*>(p)[i]);
}

__device__ __forceinline__ void ste(void* p, int dt, int64_t i, float v) {
  if (dt == 0) static_cast<float*>(p)[i] = v;
  else if (dt == 1) static_cast<__half*>(p)[i] = __float2half(v);
  else static_cast<__hip_bfloat16*>(p)[i] = __float2bfloat16(v);
}

__device__ __forceinline__ uint32_t pack2(int dt, float lo, float hi) {
  if (dt == 1) return static_cast<uint32_t>(__half_as_ushort(__float2half(lo))) |
                      (static_cast<uint32_t>(__half_as_ushort(__float2half(hi))) << 16);
  return static_cast<uint32_t>(__bfloat16_as_ushort(__float2bfloat16(lo))) |
         (static_cast<uint32_t>(__bfloat16_as_ushort(__float2bfloat16(hi))) << 16);
}

// W (4 or 8) consecutive elements from element offset i; the address is aligned to min(16, W * element size)
template <int W>
__device__ __forceinline__ void ldv(const void* p, int dt, int64_t i, float* out) {
  if (dt == 0) {
#pragma unroll
    for (int k = 0; k < W / 4; ++k) {
      const float4 t = *reinterpret_cast<const float4*>(static_cast<const float*>(p) + i + 4 * k);
      out[4 * k] = t.x; out[4 * k + 1] = t.y; out[4 * k + 2] = t.z; out[4 * k + 3] = t.w;
    }
  } else {
    using V = typename std::conditional<W == 8, uint4, uint2>::type;
    const V raw = *reinterpret_cast<const V*>(static_cast<const uint16_t*>(p) + i);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&raw);
#pragma unroll
    for (int k = 0; k < W / 2; ++k) {
      if (dt == 1) {
        out[2 * k] = __half2float(__ushort_as_half(static_cast<unsigned short>(w[k] & 0xffffu)));
        out[2 * k + 1] = __half2float(__ushort_as_half(static_cast<unsigned short>(w[k] >> 16)));
      } else {
        out[2 * k] = __uint_as_float(w[k] << 16);
        out[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
      }
    }
  }
}

template <int W>
__device__ __forceinline__ void stv(void* p, int dt, int64_t i, const float* in) {
  if (dt == 0) {
#pragma unroll
    for (int k = 0; k < W / 4; ++k)
      *reinterpret_cast<float4*>(static_cast<float*>(p) + i + 4 * k) =
          make_float4(in[4 * k], in[4 * k + 1], in[4 * k + 2], in[4 * k + 3]);
  } else {
    using V = typename std::conditional<W == 8, uint4, uint2>::type;
    V raw;
    uint32_t* w = reinterpret_cast<uint32_t*>(&raw);
#pragma unroll
    for (int k = 0; k < W / 2; ++k) w[k] = pack2(dt, in[2 * k], in[2 * k + 1]);
    *reinterpret_cast<V*>(static_cast<uint16_t*>(p) + i) = raw;
  }
}

// ---------------------------------------------------------------- reductions
template <int CTRL>
__device__ __forceinline__ float dpp_add(float s) {
  return s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), CTRL, 0xf, 0xf, false));
}

// sum over the 64 lanes of a wave, the same bits in every lane. Every lane must be active.
__device__ __forceinline__ float wave_sum(float s) {
  s = dpp_add<0xB1>(s);   // quad_perm [1, 0, 3, 2]: lane ^ 1
  s = dpp_add<0x4E>(s);   // quad_perm [2, 3, 0, 1]: lane ^ 2
  s = dpp_add<0x141>(s);  // row_half_mirror: the other quad of the 8 (its lanes agree by now)
  s = dpp_add<0x140>(s);  // row_mirror: the other half of the 16
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  return s;
}

// sum over the row's lanes; the block form exchanges the four wave sums through LDS slot `slot` (0 .. 3)
template <int LANES>
__device__ __forceinline__ float row_sum(float s, int slot) {
  s = wave_sum(s);
  if constexpr (LANES == kThreads) {
    __shared__ float red[4][4];
    if ((threadIdx.x & 63) == 0) red[slot][threadIdx.x >> 6] = s;
    __syncthreads();
    s = (red[slot][0] + red[slot][1]) + (red[slot][2] + red[slot][3]);
  }
  return s;
}

// a + b + c rounded once (up to second order): the rounding errors of the two additions are recovered
// exactly (two-sum) and added back, so the fp32 row and its sum output do not depend on a double rounding
__device__ __forceinline__ float add3(float a, float b, float c) {
  const float s = a + b, bb = s - a, e1 = (a - (s - bb)) + (b - bb);
  const float s2 = s + c, cc = s2 - s, e2 = (s - (s2 - cc)) + (c - cc);
  return s2 + (e1 + e2);
}

struct RowArgs {
  const void* x; const void* skip; const void* bias; const void* gamma; const void* beta;
  void* y; void* sum; float* mean; float* inv;
  const void* ids; const void* pos_ids; const void* seg_ids;
  const void* word; const void* pos; const void* seg;
  int64_t rows, x_rs, skip_rs, skip_rows;
  int N, rms, ids64, S, word_rows, pos_rows, seg_rows, bias_dt, gamma_dt, beta_dt;
  float eps;
};

__device__ __forceinline__ int64_t clamped_id(const void* ids, int ids64, int64_t r, int table_rows) {
  const int64_t id = ids64 ? static_cast<const int64_t*>(ids)[r] : static_cast<const int32_t*>(ids)[r];
  return id < 0 ? 0 : (id >= table_rows ? table_rows - 1 : id);
}

// SRC: 0 x[r]; 1 x[r] + skip[r % skip_rows] (+ bias); 2 word[ids[r]] + pos[pos_ids[r] | r % S] (+ seg[seg_ids[r]])
// LANES: 64 a wave per row, 256 the block per row
template <int DT, int SRC, bool VEC, int LANES>
__global__ __launch_bounds__(kThreads) void norm_rows_kernel(const RowArgs a) {
  constexpr int W = DT == 0 ? 4 : 8;                // elements per 16-byte vector
  constexpr int PER = LANES == 64 ? 16 : 32;        // elements a lane holds
  constexpr int NV = PER / W;
  constexpr int RPB = kThreads / LANES;             // rows a block works on at a time
  const int lane = threadIdx.x % LANES;
  const int N = a.N;
  // column of element i of vector j: consecutive per lane (vector form) or interleaved across lanes
  auto col = [&](int j, int i) { return VEC ? (j * LANES + lane) * W + i : (j * W + i) * LANES + lane; };
  // v[0 .. W) = vector j of the row of p that starts at element `base`; columns past N give 0
  auto fetch = [&](const void* p, int dt, int64_t base, int j, float* v) {
    if (VEC) {
      if (col(j, 0) < N) {
        ldv<W>(p, dt, base + col(j, 0), v);
      } else {
#pragma unroll
        for (int i = 0; i < W; ++i) v[i] = 0.f;
      }
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) v[i] = col(j, i) < N ? lde(p, dt, base + col(j, i)) : 0.f;
    }
  };

  // the wave form keeps the per-column parameters in registers across its rows
  float g[LANES == 64 ? PER : 1], b[LANES == 64 ? PER : 1], bs[LANES == 64 ? PER : 1];
  if (LANES == 64) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (a.gamma) fetch(a.gamma, a.gamma_dt, 0, j, &g[j * W]);
      if (a.beta) fetch(a.beta, a.beta_dt, 0, j, &b[j * W]);
      if (SRC == 1 && a.bias) fetch(a.bias, a.bias_dt, 0, j, &bs[j * W]);
    }
  }

  int it = 0;  // the block form alternates its LDS slots, so a slow wave never reads what the next row wrote
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / LANES; r < a.rows;
       r += static_cast<int64_t>(gridDim.x) * RPB, ++it) {
    float v[PER];
    if (SRC == 2) {
      const int64_t wi = clamped_id(a.ids, a.ids64, r, a.word_rows);
      int64_t pi = a.pos_ids ? clamped_id(a.pos_ids, a.ids64, r, a.pos_rows) : r % a.S;
      pi = pi >= a.pos_rows ? a.pos_rows - 1 : pi;
      const int64_t si = a.seg_ids ? clamped_id(a.seg_ids, a.ids64, r, a.seg_rows) : 0;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        float t[W], u[W] = {};
        fetch(a.word, DT, wi * N, j, &v[j * W]);
        fetch(a.pos, DT, pi * N, j, t);
        if (a.seg_ids) fetch(a.seg, DT, si * N, j, u);
#pragma unroll
        for (int i = 0; i < W; ++i) v[j * W + i] = a.seg_ids ? add3(v[j * W + i], t[i], u[i]) : v[j * W + i] + t[i];
      }
    } else {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        fetch(a.x, DT, r * a.x_rs, j, &v[j * W]);
        if (SRC == 1) {
          float t[W], u[W] = {};
          fetch(a.skip, DT, (r % a.skip_rows) * a.skip_rs, j, t);
          if constexpr (LANES != 64) {
            if (a.bias) fetch(a.bias, a.bias_dt, 0, j, u);
          }
#pragma unroll
          for (int i = 0; i < W; ++i) {
            float c = 0.f;
            if constexpr (LANES == 64) c = bs[j * W + i]; else c = u[i];
            v[j * W + i] = a.bias ? add3(v[j * W + i], t[i], c) : v[j * W + i] + t[i];
          }
        }
      }
    }
    if (a.sum) {  // the un-normalised row, rounded once from the fp32 sum
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        if (VEC) {
          if (col(j, 0) < N) stv<W>(a.sum, DT, r * N + col(j, 0), &v[j * W]);
        } else {
#pragma unroll
          for (int i = 0; i < W; ++i)
            if (col(j, i) < N) ste(a.sum, DT, r * N + col(j, i), v[j * W + i]);
        }
      }
    }

    float s = 0.f;
    if (!a.rms) {
#pragma unroll
      for (int k = 0; k < PER; ++k) s += v[k];  // lanes past N hold 0
      s = row_sum<LANES>(s, it & 1);
    }
    const float mean = s / static_cast<float>(N);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const float d = v[j * W + i] - mean;
        if (col(j, VEC ? 0 : i) < N) q += d * d;  // masked, not (0 - mean)^2
      }
    q = row_sum<LANES>(q, 2 + (it & 1));
    const float inv = 1.f / sqrtf(q / static_cast<float>(N) + a.eps);
    if (lane == 0) {
      if (a.mean) a.mean[r] = mean;
      if (a.inv) a.inv[r] = inv;
    }

#pragma unroll
    for (int j = 0; j < NV; ++j) {
      float gj[W], bj[W], o[W];
      if (LANES != 64) {
        if (a.gamma) fetch(a.gamma, a.gamma_dt, 0, j, gj);
        if (a.beta) fetch(a.beta, a.beta_dt, 0, j, bj);
      }
#pragma unroll
      for (int i = 0; i < W; ++i) {
        float t = (v[j * W + i] - mean) * inv;
        if constexpr (LANES == 64) {
          if (a.gamma) t *= g[j * W + i];
          if (a.beta) t += b[j * W + i];
        } else {
          if (a.gamma) t *= gj[i];
          if (a.beta) t += bj[i];
        }
        o[i] = t;
      }
      if (VEC) {
        if (col(j, 0) < N) stv<W>(a.y, DT, r * N + col(j, 0), o);
      } else {
#pragma unroll
        for (int i = 0; i < W; ++i)
          if (col(j, i) < N) ste(a.y, DT, r * N + col(j, i), o[i]);
      }
    }
  }
}

// ---------------------------------------------------------------- bias + activation
// mode 0: erf GELU, 0.5 v erfc(-v / sqrt 2) (no 1 + erf cancellation for negative v); 1: tanh GELU,
// 0.5 v (1 + tanh u) = v / (1 + exp(-2 u)), u = sqrt(2 / pi) (v + 0.044715 v^3); 2: v sigmoid(alpha v).
// HALF (fp16 / bf16 results): the erf form is 0.5 v (1 + erf(v / sqrt 2)); its absolute error of about
// |v| 2^-25 in the negative tail is far below a 16-bit result's rounding where the result matters, and erff
// costs about half of erfcf, which the 16-bit kernel (twice the math per byte) is bound by.
template <bool HALF>
__device__ __forceinline__ float act_gelu(float v, int mode, float alpha) {
  if (mode == 0)
    return HALF ? 0.5f * v * (1.f + erff(0.70710678118654752f * v)) : 0.5f * v * erfcf(-0.70710678118654752f * v);
  const float z = mode == 1 ? 1.5957691216057308f * (v + 0.044715f * v * v * v) : alpha * v;
  return v / (1.f + expf(-z));
}

template <int DT, bool VEC>
__global__ __launch_bounds__(kThreads) void bias_act_kernel(const void* __restrict__ x, int64_t x_rs,
                                                            const void* __restrict__ bias, int bias_dt,
                                                            void* __restrict__ y, int64_t rows, int N, int mode,
                                                            float alpha) {
  constexpr int W = DT == 0 ? 4 : 8;
  constexpr int UNR = 2;  // two 16-byte vectors per thread, both loads in flight before the math
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  if (VEC) {
    const int vpr = N / W;
    const int64_t total = rows * vpr;
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; t * UNR < total; t += stride) {
      float v[UNR][W], bv[UNR][W];
      int64_t r[UNR];
      int c[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int64_t g = t * UNR + u;
        if (g < total) {
          r[u] = g / vpr;
          c[u] = static_cast<int>(g - r[u] * vpr) * W;
          ldv<W>(x, DT, r[u] * x_rs + c[u], v[u]);
          if (bias) ldv<W>(bias, bias_dt, c[u], bv[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (t * UNR + u < total) {
#pragma unroll
          for (int i = 0; i < W; ++i) v[u][i] = act_gelu<DT != 0>(bias ? v[u][i] + bv[u][i] : v[u][i], mode, alpha);
          stv<W>(y, DT, r[u] * N + c[u], v[u]);
        }
      }
    }
  } else {
    const int64_t total = rows * N;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; e < total; e += stride) {
      const int64_t r = e / N;
      const int c = static_cast<int>(e - r * N);
      float v = lde(x, DT, r * x_rs + c);
      if (bias) v += lde(bias, bias_dt, c);
      ste(y, DT, e, act_gelu<DT != 0>(v, mode, alpha));
    }
  }
}

// CUs of the current device (the caller launches on one of its streams)
int cu_count() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
    (void)hipGetLastError();
    v = 256;
  }
  return v;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
bool dt_ok(int dt) { return dt >= 0 && dt <= 2; }

template <int DT, int SRC>
void launch_rows(const RowArgs& a, bool vec, hipStream_t s) {
  const bool wave = a.N <= kWaveMaxN;
  const int64_t blocks = wave ? (a.rows + 3) / 4 : a.rows;
  const int grid = static_cast<int>(std::min<int64_t>(blocks, static_cast<int64_t>(cu_count()) * 8));
  if (wave) {
    if (vec) hipLaunchKernelGGL((norm_rows_kernel<DT, SRC, true, 64>), dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((norm_rows_kernel<DT, SRC, false, 64>), dim3(grid), dim3(kThreads), 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((norm_rows_kernel<DT, SRC, true, 256>), dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((norm_rows_kernel<DT, SRC, false, 256>), dim3(grid), dim3(kThreads), 0, s, a);
  }
}

template <int DT>
void launch_rows_src(const RowArgs& a, int src, bool vec, hipStream_t s) {
  if (src == 0) launch_rows<DT, 0>(a, vec, s);
  else if (src == 1) launch_rows<DT, 1>(a, vec, s);
  else launch_rows<DT, 2>(a, vec, s);
}

}  // namespace

int NormRows(const NormRowsArgs& n, int dtype, void* stream) {
  const bool gather = n.word != nullptr;
  if (!dt_ok(dtype) || n.rows <= 0 || n.N <= 0 || n.N > kBlockMaxN || !n.y) return -4;
  if (!dt_ok(n.bias_dt) || !dt_ok(n.gamma_dt) || !dt_ok(n.beta_dt)) return -4;
  if (gather) {
    if (n.x || n.skip || n.bias || !n.ids || !n.pos || n.word_rows <= 0 || n.pos_rows <= 0 || n.S <= 0) return -4;
    if ((n.seg_ids != nullptr) != (n.seg != nullptr) || (n.seg && n.seg_rows <= 0)) return -4;
  } else {
    if (!n.x || n.x_rs < 0 || (n.bias && !n.skip)) return -4;
    if (n.skip && (n.skip_rows <= 0 || n.skip_rs < 0)) return -4;
  }
  if (n.rms && (n.beta || n.mean)) return -4;
  const int esz = dtype == 0 ? 4 : 2, W = 16 / esz;
  bool vec = n.N % W == 0 && aligned16(n.y) && aligned16(n.sum) && aligned16(n.gamma) && aligned16(n.beta);
  if (gather) {
    vec = vec && aligned16(n.word) && aligned16(n.pos) && aligned16(n.seg);
  } else {
    vec = vec && aligned16(n.x) && (n.x_rs * esz) % 16 == 0 && aligned16(n.skip) && (n.skip_rs * esz) % 16 == 0 &&
          aligned16(n.bias);
  }
  RowArgs a;
  a.x = n.x; a.skip = n.skip; a.bias = n.bias; a.gamma = n.gamma; a.beta = n.beta;
  a.y = n.y; a.sum = n.sum; a.mean = n.mean; a.inv = n.inv;
  a.ids = n.ids; a.pos_ids = n.pos_ids; a.seg_ids = n.seg_ids; a.word = n.word; a.pos = n.pos; a.seg = n.seg;
  a.rows = n.rows; a.x_rs = n.x_rs; a.skip_rs = n.skip_rs; a.skip_rows = n.skip ? n.skip_rows : 1;
  a.N = n.N; a.rms = n.rms; a.ids64 = n.ids64; a.S = n.S;
  a.word_rows = n.word_rows; a.pos_rows = n.pos_rows; a.seg_rows = n.seg_rows;
  a.bias_dt = n.bias_dt; a.gamma_dt = n.gamma_dt; a.beta_dt = n.beta_dt; a.eps = n.eps;
  const int src = gather ? 2 : (n.skip ? 1 : 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == 0) launch_rows_src<0>(a, src, vec, s);
  else if (dtype == 1) launch_rows_src<1>(a, src, vec, s);
  else launch_rows_src<2>(a, src, vec, s);
  NR_HIP_CHECK(hipGetLastError());
  return 0;
}

int BiasAct(const void* x, int64_t x_rs, const void* bias, int bias_dt, void* y, int64_t rows, int N, int mode,
            float alpha, int dtype, void* stream) {
  if (!dt_ok(dtype) || !dt_ok(bias_dt) || rows <= 0 || N <= 0 || !x || !y || x_rs < 0 || mode < 0 || mode > 2)
    return -4;
  const int esz = dtype == 0 ? 4 : 2, W = 16 / esz;
  const bool vec = N % W == 0 && aligned16(x) && aligned16(y) && aligned16(bias) && (x_rs * esz) % 16 == 0;
  const int64_t threads = vec ? (rows * (N / W) + 1) / 2 : rows * N;
  const int grid = static_cast<int>(
      std::min<int64_t>((threads + kThreads - 1) / kThreads, static_cast<int64_t>(cu_count()) * 16));
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto go = [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (vec) hipLaunchKernelGGL((bias_act_kernel<DT, true>), dim3(grid), dim3(kThreads), 0, s, x, x_rs, bias, bias_dt,
                                y, rows, N, mode, alpha);
    else hipLaunchKernelGGL((bias_act_kernel<DT, false>), dim3(grid), dim3(kThreads), 0, s, x, x_rs, bias, bias_dt,
                            y, rows, N, mode, alpha);
  };
  if (dtype == 0) go(std::integral_constant<int, 0>{});
  else if (dtype == 1) go(std::integral_constant<int, 1>{});
  else go(std::integral_constant<int, 2>{});
  NR_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace smlnn
