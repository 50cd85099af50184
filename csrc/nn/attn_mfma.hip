// K22: fused online-softmax ("flash") attention forward on the CDNA4 16x16x32 f16 / bf16 matrix cores
// (module _nn; com.microsoft Attention / MultiHeadAttention of the ONNX executor).
//
//   out[b, s, h, :] = softmax_l(scale * q[b,s,h,:] . k[b,l,h,:] + key_add[b,l] + bias[b,h,s,l] + causal(s,l))
//                     . v[b,l,h,:]
//
// q, k, v are read in place through element strides (batch, row, head; unit stride along the head
// dimension), so the slices of a packed QKV projection and past-concatenated K / V need no copy. The
// [S, L] score matrix never exists in memory. Head sizes 32, 64 and 128 are compiled; 96 is declined.
//
// Work split: grid (query tiles of 64, heads, batch); 256 threads = 4 waves, each wave owns 16 queries.
// The waves share key tiles of 64: K as [key][d] at a pitch of 2 d + 32 bytes and V transposed as
// [d][key] at a pitch of 160 bytes, both double-buffered in LDS (d = 128: 76 KiB, two blocks per CU); the
// 16-byte buffer loads of tile t + 1 are issued before the MFMAs of tile t and written to the other
// buffer after them, one barrier per tile. Both pitches are an odd multiple of 32 bytes, which keeps
// the 16-lane ds_read_b128 fragment reads conflict-free (the pitch conv_mfma and qgemm_mfma measured).
// Rows past S or L are zero-filled by the buffer resource; nothing is padded in memory.
//
// Scores are computed transposed, S^T = K . Q^T: K (rows = keys) is the first MFMA operand, Q (columns =
// queries) the second, its fragments loaded once from global memory and kept in registers. In the
// accumulator layout a lane then holds, for query lane % 16, keys 16 j + 4 (lane / 16) + 0..3 of each
// 16-key sub-tile j: the row max is 15 register maxima and two cross-lane steps (lane ^ 16, lane ^ 32);
// the running max m and the rescale factor are one scalar per lane. The row sum l stays a per-lane
// partial (the four lanes of a query share m, so they rescale alike) and is reduced once at the end; it
// is summed from the fp32 p before they are rounded. exp is v_exp_f32 on scores pre-multiplied by
// log2(e), the additive terms scaled alike. A running max of -inf (a causal tile hidden for that row) is
// replaced by 0 in the exponent, so the rescale is exp2(-inf) = 0 and never NaN.
//
// P goes to f16 / bf16 in registers and is the second operand of O^T = V^T . P^T directly: MFMA k index
// 8 g + e of a lane (g = lane / 16) is key 4 g + e of sub-tile 2 t for e < 4 and key 4 g + e - 4 of
// sub-tile 2 t + 1 for e >= 4. V is transposed at the LDS write into that same permuted key order, so its
// fragment is again one ds_read_b128: a thread loads the same 8 head-dim elements of keys 2 m and
// 2 m + 1 (adjacent in the permuted order too) and writes 8 packed dwords. This was chosen over the
// transposing LDS reads: it keeps every fragment read a b128 at the measured pitch, and the dword
// writes of a wave cover whole 128-byte rows. O^T leaves a lane 4 consecutive head-dim elements of one
// query: scaled by 1 / l, one 8-byte store. Causal: key l is visible to query s iff l <= s + (L - S);
// key tiles above the block's diagonal are not visited, and a wave skips the MFMAs of a tile above its
// own. No register spills for any head size.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "nn_ops.h"

namespace smlnn {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kBQ = 64, kBL = 64;  // queries per block, keys per tile
constexpr int kPV = 160;           // pitch of a V^T row (64 keys) in bytes
constexpr float kLog2e = 1.4426950408889634f;
constexpr uint32_t kOob = 0x80000000u;  // past every buffer resource's range: the load returns zero

__device__ __forceinline__ uint4 Load16(__amdgpu_buffer_rsrc_t rsrc, uint32_t off) {
  auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
  uint4 r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}

template <typename T, int D>
__global__ __launch_bounds__(kThreads) void attn_mfma_kernel(AttnArgs a) {
  typedef typename std::conditional<std::is_same<T, _Float16>::value, h8, b8>::type V8;
  constexpr int PK = 2 * D + 32;          // pitch of a K row in bytes
  constexpr int KS = D / 32, DT = D / 16;  // MFMA k steps of Q.K; 16-row sub-tiles of O^T
  constexpr int CR = D / 8;                // 16-byte chunks per row
  constexpr int NV = D >= 64 ? D / 64 : 1, VI = 4 * D;  // V work items per thread, per tile
  constexpr int KB = kBL * PK, VB = D * kPV;
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * (KB + VB)];
  uint8_t* Ks = lds;
  uint8_t* Vs = lds + 2 * KB;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int q0 = blockIdx.x * kBQ, h = blockIdx.y, b = blockIdx.z;
  const int S = a.S, L = a.L, diag = L - S;
  const int qrow = q0 + wid * 16 + fr;  // this lane's query

  const T* qp = static_cast<const T*>(a.q) + b * a.q_sb + h * a.q_sh;
  const T* kp = static_cast<const T*>(a.k) + b * a.k_sb + h * a.k_sh;
  const T* vp = static_cast<const T*>(a.v) + b * a.v_sb + h * a.v_sh;
  const auto rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(qp), 0,
                                                    static_cast<int>(((S - 1) * a.q_sr + D) * 2), 0x00020000);
  const auto rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(kp), 0,
                                                    static_cast<int>(((L - 1) * a.k_sr + D) * 2), 0x00020000);
  const auto rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(vp), 0,
                                                    static_cast<int>(((L - 1) * a.v_sr + D) * 2), 0x00020000);
  const uint32_t ksr = static_cast<uint32_t>(a.k_sr) * 2, vsr = static_cast<uint32_t>(a.v_sr) * 2;

  // Q fragments: query lane % 16, head-dim elements 32 ks + 8 (lane / 16) .. + 7
  V8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const uint32_t off = qrow < S ? static_cast<uint32_t>(qrow * a.q_sr * 2) + ks * 64 + fg * 16 : kOob;
    const uint4 w = Load16(rq, off);
    __builtin_memcpy(&qf[ks], &w, 16);
  }

  // key tiles the block visits: causal stops at the diagonal of its last query
  int kend = L;
  if (a.causal) {
    const int qlast = q0 + kBQ - 1 < S - 1 ? q0 + kBQ - 1 : S - 1;
    kend = qlast + diag + 1 < L ? qlast + diag + 1 : L;
  }
  const int nt = (kend + kBL - 1) / kBL;

  uint4 kreg[KS], vreg[NV][2];
  auto load_tile = [&](int k0) {
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const int c = tid + kThreads * i;
      const int key = k0 + c / CR;
      kreg[i] = Load16(rk, key < L ? key * ksr + (c % CR) * 16 : kOob);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int w = tid + kThreads * i;
      const int key = k0 + 2 * (w & 31), ch = w >> 5;
      const bool on = w < VI;
      vreg[i][0] = Load16(rv, on && key < L ? key * vsr + ch * 16 : kOob);
      vreg[i][1] = Load16(rv, on && key + 1 < L ? (key + 1) * vsr + ch * 16 : kOob);
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const int c = tid + kThreads * i;
      *reinterpret_cast<uint4*>(Ks + buf * KB + (c / CR) * PK + (c % CR) * 16) = kreg[i];
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int w = tid + kThreads * i;
      if (w >= VI) continue;
      // keys kk, kk + 1 of the tile -> permuted position 32 t + 8 g + 4 hi + e (kk = 32 t + 16 hi + 4 g + e)
      const int kk = 2 * (w & 31), ch = w >> 5;
      const int pos = (kk & 32) + 8 * ((kk >> 2) & 3) + 4 * ((kk >> 4) & 1) + (kk & 3);
      uint8_t* dst = Vs + buf * VB + (8 * ch) * kPV + pos * 2;
      const uint32_t lo[4] = {vreg[i][0].x, vreg[i][0].y, vreg[i][0].z, vreg[i][0].w};
      const uint32_t hi[4] = {vreg[i][1].x, vreg[i][1].y, vreg[i][1].z, vreg[i][1].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        *reinterpret_cast<uint32_t*>(dst + (2 * j) * kPV) = (lo[j] & 0xffffu) | (hi[j] << 16);
        *reinterpret_cast<uint32_t*>(dst + (2 * j + 1) * kPV) = (lo[j] >> 16) | (hi[j] & 0xffff0000u);
      }
    }
  };

  f4 o[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) o[i] = f4{0.f, 0.f, 0.f, 0.f};
  const float ninf = -__builtin_inff();
  float m_run = ninf, l_run = 0.f;
  const float sc2 = a.scale * kLog2e;
  const float* ka = a.key_add ? a.key_add + static_cast<int64_t>(b) * L : nullptr;
  const float* bi = a.bias && qrow < S ? a.bias + b * a.bias_sb + h * a.bias_sh + qrow * a.bias_sr : nullptr;

  auto compute = [&](int buf, int k0) {
    const uint8_t* kt = Ks + buf * KB;
    const uint8_t* vt = Vs + buf * VB;
    f4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const V8 kf = *reinterpret_cast<const V8*>(kt + (16 * j + fr) * PK + ks * 64 + fg * 16);
        if constexpr (std::is_same<T, _Float16>::value)
          s[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], s[j], 0, 0, 0);
        else
          s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[j], 0, 0, 0);
      }
    }
    // lane: query qrow, keys k0 + 16 j + 4 fg + r
    float x[4][4];
    float mx = ninf;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + 16 * j + 4 * fg + r;
        float t = s[j][r] * sc2;
        if (key < L) {
          if (ka) t += ka[key] * kLog2e;
          if (bi) t += bi[key] * kLog2e;
        }
        if (key >= L || (a.causal && key > qrow + diag)) t = ninf;
        x[j][r] = t;
        mx = fmaxf(mx, t);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float m_use = m_new == ninf ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        x[j][r] = __builtin_amdgcn_exp2f(x[j][r] - m_use);
        psum += x[j][r];
      }
    l_run = l_run * alpha + psum;
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[i][r] *= alpha;
    V8 pf[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e) pf[t][e] = static_cast<T>(x[2 * t + (e >> 2)][e & 3]);
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const V8 vf = *reinterpret_cast<const V8*>(vt + (16 * i + fr) * kPV + (32 * t + 8 * fg) * 2);
        if constexpr (std::is_same<T, _Float16>::value)
          o[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[t], o[i], 0, 0, 0);
        else
          o[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[t], o[i], 0, 0, 0);
      }
  };

  load_tile(0);
  store_tile(0);
  __syncthreads();
  const int wave_last = q0 + wid * 16 + 15 + diag;  // last key any query of this wave sees when causal
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) load_tile((t + 1) * kBL);
    if (!(a.causal && t * kBL > wave_last)) compute(buf, t * kBL);
    if (t + 1 < nt) store_tile(buf ^ 1);
    __syncthreads();
  }

  // lane: head-dim elements 16 i + 4 fg + 0..3 of query qrow
  float l = l_run;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  const float inv = 1.f / l;
  if (qrow < S) {
    T* op = static_cast<T*>(a.out) + ((static_cast<int64_t>(b) * S + qrow) * a.heads + h) * D + 4 * fg;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      T w[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) w[r] = static_cast<T>(o[i][r] * inv);
      uint2 pk;
      __builtin_memcpy(&pk, w, 8);
      *reinterpret_cast<uint2*>(op + 16 * i) = pk;
    }
  }
}

template <typename T>
int LaunchAttn(const AttnArgs& a, hipStream_t st) {
  const dim3 grid((a.S + kBQ - 1) / kBQ, a.heads, a.B);
  if (a.d == 32) hipLaunchKernelGGL((attn_mfma_kernel<T, 32>), grid, dim3(kThreads), 0, st, a);
  else if (a.d == 64) hipLaunchKernelGGL((attn_mfma_kernel<T, 64>), grid, dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL((attn_mfma_kernel<T, 128>), grid, dim3(kThreads), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

bool Aligned16(const void* p, int64_t sb, int64_t sr, int64_t sh) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0 && sb % 8 == 0 && sr % 8 == 0 && sh % 8 == 0;
}

}  // namespace

int AttnMfma(const AttnArgs& a, int dtype, void* stream) {
  if (a.B <= 0 || a.heads <= 0 || a.S <= 0) return 0;
  if (dtype != 1 && dtype != 2) return -2;
  if (!a.q || !a.k || !a.v || !a.out || a.L <= 0) return -2;
  // not taken (the caller keeps its own path): head size, causal with fewer keys than queries, grid limits,
  // operands the 16-byte loads cannot read in place
  if (a.d != 32 && a.d != 64 && a.d != 128) return -4;
  if (a.causal && a.L < a.S) return -4;
  if (a.B > 65535 || a.heads > 65535) return -4;
  if (!Aligned16(a.q, a.q_sb, a.q_sr, a.q_sh) || !Aligned16(a.k, a.k_sb, a.k_sr, a.k_sh) ||
      !Aligned16(a.v, a.v_sb, a.v_sr, a.v_sh))
    return -4;
  if (a.q_sr < 0 || a.k_sr < 0 || a.v_sr < 0) return -4;
  // 32-bit byte offsets inside one (batch, head) slice
  const int64_t lim = 1ll << 30;
  if ((a.S - 1) * a.q_sr + a.d >= lim || (a.L - 1) * a.k_sr + a.d >= lim || (a.L - 1) * a.v_sr + a.d >= lim)
    return -5;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == 1 ? LaunchAttn<_Float16>(a, st) : LaunchAttn<__bf16>(a, st);
}

}  // namespace smlnn
