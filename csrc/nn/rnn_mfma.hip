// K24: fused persistent LSTM / GRU on the CDNA4 fp32 matrix cores (module _nn; the device path of the ONNX
// LSTM and GRU operators).
//
//   one launch runs all T steps of every direction: it reads the precomputed input projection XW (with the
//   biases the step adds before its activations) and writes Y, Y_h and, for LSTM, Y_c
//
// Work split: grid (batch tiles of 16 items, directions). The recurrence of an item depends on no other item,
// so a block keeps the state of its 16 items on chip for the whole sequence and never talks to another block:
// no grid sync, no cooperative launch, no wait on memory; every loop is bounded by T, the tile count or H / 16.
//
// Matrix instruction: v_mfma_f32_16x16x4_f32 with a 16 x 4 piece of R as the first operand and 4 x 16 of
// h^T (k x items) as the second: a lane's four accumulator values are hidden units 4 (lane / 16) + 0..3 of a
// 16-unit tile for the one item lane % 16. A wave owns whole unit tiles (tile u = wave + slot * waves: one slot
// on up to 16 waves for H <= 256, four slots on up to 8 waves, which leaves a wave 256 registers, for H <= 512)
// and computes every gate of a tile, so all gate pre-activations of a (unit, item) pair meet in one lane: the
// cell update is register arithmetic, the LSTM cell state never leaves its registers between step 0 and step T.
// A block streams all of R once per step through one CU, about 45 GB/s measured, so a step costs about
// 25 us at H = 256 and 87 us at H = 512; beyond that the unfused time loop (about 170 us per step whatever the
// size) wins, measured 0.72x at H = 640 and 0.53x at H = 1024, and such sizes are declined.
//
// R: no two waves need the same rows, so R is not staged in LDS. The Python side repacks it once per call in
// fragment order [direction][unit tile][gate][k chunk of 16][lane][4], zero-padded to Hp = H rounded up to 16:
// a lane's operand of four consecutive MFMAs is one coalesced 16-byte global load, issued one k chunk ahead of
// the MFMAs that use it. MFMA i of a chunk multiplies column 16 kc + 4 (lane / 16) + i: the same permutation
// of the k index for both operands, as in mips_topk.
//
// h: the shared second operand, [16 items][Hp + 8] floats in LDS (a row pitch that is an odd multiple of 32
// bytes: conflict-free for the 16-lane ds_read_b128). LSTM and GRU with linear_before_reset = 1 double-buffer
// it by step parity: one barrier per step. GRU with linear_before_reset = 0 needs (r . h) Rh^T: phase 1
// computes z and r of every tile and writes r . h to the second buffer, a barrier, phase 2 runs the h gate
// against it and updates h in place (in phase 2 a lane reads and writes only its own units of h), a barrier.
//
// XW [direction][T][N][gates * Hp] holds Wb and every part of Rb that is added before an activation; only the
// Rbh of linear_before_reset = 1, which sits inside r . (...), is read by the kernel. A pass loads its slice
// (16 bytes per lane and gate) before its MFMAs and adds it after them, so the load hides under them.
//
// Lengths: an item walks time index step (forward) or len - 1 - step (reverse) while step < len; afterwards
// its state is frozen and zeros are written to Y[step], which are exactly the rows past its length: Y needs no
// clearing. Y_h / Y_c are the frozen state; a length of 0 returns the initial state. Nothing on the launch
// path reads a tensor value.
//
// LDS: 2 x 16 x (Hp + 8) x 4 bytes (dynamic): 3 KiB at H = 16, 65 KiB at H = 512. No scratch in any form.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nn_ops.h"

namespace smlnn {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kMaxWaves = 16;  // one tile slot per wave; 8 waves with four slots
constexpr int kMaxHidden = 512;
constexpr int kPad = 8;  // floats added to an LDS row of Hp

__device__ __forceinline__ float Sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }
// (1 - e) / (1 + e) with e = exp(-2 |x|) in (0, 1]: no overflow, absolute error of a few ulp of 1
__device__ __forceinline__ float Tanh(float x) {
  const float e = __expf(-2.0f * __builtin_fabsf(x));
  return __builtin_copysignf((1.0f - e) / (1.0f + e), x);
}
__device__ __forceinline__ float Clip(float x, float c) {
  return c > 0.f ? __builtin_fminf(__builtin_fmaxf(x, -c), c) : x;
}

// acc[g] += R(tile, gate g) . h over all KC k chunks. rp: the lane's 16 bytes of (gate 0, chunk 0); a gate is
// gs floats further, a chunk 256. hrow: the lane's 16 bytes of chunk 0 in LDS (item row + 4 (lane / 16)).
template <int G>
__device__ __forceinline__ void TileGemm(f4 (&acc)[G], const float* __restrict__ rp, int gs, const float* hrow,
                                         int KC) {
  f4 rc[G], rn[G];
#pragma unroll
  for (int g = 0; g < G; ++g) rc[g] = *reinterpret_cast<const f4*>(rp + g * gs);
  f4 hc = *reinterpret_cast<const f4*>(hrow);
  for (int kc = 0; kc < KC; ++kc) {
    const int nk = kc + 1 < KC ? kc + 1 : kc;  // the last chunk reloads itself
#pragma unroll
    for (int g = 0; g < G; ++g) rn[g] = *reinterpret_cast<const f4*>(rp + g * gs + nk * 256);
    const f4 hn = *reinterpret_cast<const f4*>(hrow + nk * 16);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(rc[g][i], hc[i], acc[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G; ++g) rc[g] = rn[g];
    hc = hn;
  }
}

// CELL: 0 LSTM (gates i, o, f, c), 1 GRU linear_before_reset = 1, 2 GRU linear_before_reset = 0 (gates z, r, h)
template <int CELL, int TPW>
__global__ __launch_bounds__(TPW == 1 ? 1024 : 512) void rnn_kernel(RnnArgs a, int Hp, int NW) {
  extern __shared__ __attribute__((aligned(16))) float rnn_lds[];
  constexpr int G = CELL == 0 ? 4 : 3;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int T = a.T, N = a.N, H = a.H, d = blockIdx.y;
  const int KC = Hp >> 4, pitch = Hp + kPad, gs = KC * 256;
  const int n = blockIdx.x * 16 + fr;
  const bool live = n < N;
  const int nc = live ? n : N - 1;  // lanes past N read the last item and store nothing
  int len = T;
  if (a.lens) len = a.lens[nc];
  len = len < 0 ? 0 : (len > T ? T : len);
  if (!live) len = 0;
  const bool rev = (a.reverse >> d) & 1;
  const bool vec = (H & 3) == 0;  // 16-byte stores to Y / Y_h / Y_c
  const float clip = a.clip;

  float* const hb0 = rnn_lds;
  float* const hb1 = rnn_lds + 16 * pitch;
  const int64_t sbase = static_cast<int64_t>(d) * N * H;  // of [nd][N][H] states
  for (int i = tid; i < 16 * Hp; i += NW * 64) {
    const int it = i / Hp, col = i - it * Hp, nn = blockIdx.x * 16 + it;
    hb0[it * pitch + col] = a.h0 && nn < N && col < H ? a.h0[sbase + static_cast<int64_t>(nn) * H + col] : 0.f;
  }
  // this lane's units of slot j: 16 (wid + j NW) + 4 fg + 0..3
  const int col0 = wid * 16 + fg * 4;
  f4 c[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    c[j] = f4{0.f, 0.f, 0.f, 0.f};
    if (CELL == 0 && a.c0 && live) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int unit = col0 + j * NW * 16 + i;
        if (unit < H) c[j][i] = a.c0[sbase + static_cast<int64_t>(n) * H + unit];
      }
    }
  }
  __syncthreads();

  const float* const rdir = a.r + static_cast<int64_t>(d) * G * Hp * Hp + lane * 4;
  const float* const xdir = a.xw + static_cast<int64_t>(d) * T * N * G * Hp;
  auto store4 = [&](float* p, int col, f4 v) {  // p: the row of H floats; units col .. col + 3
    if (vec) {
      if (col < H) *reinterpret_cast<f4*>(p + col) = v;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (col + i < H) p[col + i] = v[i];
    }
  };

  for (int step = 0; step < T; ++step) {
    const bool valid = step < len;
    const int t = valid ? (rev ? len - 1 - step : step) : step;  // the row of Y this lane writes
    const float* const xrow = xdir + (static_cast<int64_t>(valid ? t : 0) * N + nc) * (G * Hp);
    float* const yrow = a.y + ((static_cast<int64_t>(t) * a.nd + d) * N + nc) * H;
    const float* const hcur = CELL == 2 ? hb0 : ((step & 1) ? hb1 : hb0);
    float* const hnxt = CELL == 2 ? hb0 : ((step & 1) ? hb0 : hb1);

    if constexpr (CELL == 2) {
      f4 z[TPW];
#pragma unroll
      for (int j = 0; j < TPW; ++j) {  // phase 1: z, r; r . h -> hb1
        const int u = wid + j * NW, col = col0 + j * NW * 16;
        if (u >= KC) break;
        f4 xw[2], acc[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          xw[g] = *reinterpret_cast<const f4*>(xrow + g * Hp + col);
          acc[g] = f4{0.f, 0.f, 0.f, 0.f};
        }
        TileGemm<2>(acc, rdir + static_cast<int64_t>(u) * G * gs, gs, hb0 + fr * pitch + fg * 4, KC);
        const f4 hold = *reinterpret_cast<const f4*>(hb0 + fr * pitch + col);
        f4 rh;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          z[j][i] = Sigmoid(Clip(acc[0][i] + xw[0][i], clip));
          rh[i] = Sigmoid(Clip(acc[1][i] + xw[1][i], clip)) * hold[i];
        }
        *reinterpret_cast<f4*>(hb1 + fr * pitch + col) = rh;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < TPW; ++j) {  // phase 2: the h gate against r . h, h updated in place
        const int u = wid + j * NW, col = col0 + j * NW * 16;
        if (u >= KC) break;
        f4 acc[1] = {f4{0.f, 0.f, 0.f, 0.f}};
        const f4 xh = *reinterpret_cast<const f4*>(xrow + 2 * Hp + col);
        TileGemm<1>(acc, rdir + (static_cast<int64_t>(u) * G + 2) * gs, gs, hb1 + fr * pitch + fg * 4, KC);
        const f4 hold = *reinterpret_cast<const f4*>(hb0 + fr * pitch + col);
        f4 hout, yv;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float hh = Tanh(Clip(acc[0][i] + xh[i], clip));
          const float hn = (1.0f - z[j][i]) * hh + z[j][i] * hold[i];
          hout[i] = valid ? hn : hold[i];
          yv[i] = valid ? hn : 0.f;
        }
        *reinterpret_cast<f4*>(hb0 + fr * pitch + col) = hout;
        if (live) store4(yrow, col, yv);
      }
    } else {
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        const int u = wid + j * NW, col = col0 + j * NW * 16;
        if (u >= KC) break;
        f4 xw[G], acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          xw[g] = *reinterpret_cast<const f4*>(xrow + g * Hp + col);
          acc[g] = f4{0.f, 0.f, 0.f, 0.f};
        }
        f4 p[3];  // LSTM: peepholes i, o, f; GRU: p[0] = Rbh
#pragma unroll
        for (int g = 0; g < 3; ++g) p[g] = f4{0.f, 0.f, 0.f, 0.f};
        if constexpr (CELL == 0) {
          if (a.peep) {
#pragma unroll
            for (int g = 0; g < 3; ++g)
              p[g] = *reinterpret_cast<const f4*>(a.peep + (static_cast<int64_t>(d) * 3 + g) * Hp + col);
          }
        } else {
          if (a.rbh) p[0] = *reinterpret_cast<const f4*>(a.rbh + static_cast<int64_t>(d) * Hp + col);
        }
        TileGemm<G>(acc, rdir + static_cast<int64_t>(u) * G * gs, gs, hcur + fr * pitch + fg * 4, KC);
        const f4 hold = *reinterpret_cast<const f4*>(hcur + fr * pitch + col);
        f4 hout, yv;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float hn;
          if constexpr (CELL == 0) {
            const float zi = Clip(acc[0][i] + xw[0][i], clip), zo = Clip(acc[1][i] + xw[1][i], clip);
            const float zf = Clip(acc[2][i] + xw[2][i], clip), zc = Clip(acc[3][i] + xw[3][i], clip);
            const float cold = c[j][i];
            const float ig = Sigmoid(zi + p[0][i] * cold);
            const float fgt = a.coupled ? 1.0f - ig : Sigmoid(zf + p[2][i] * cold);
            const float cn = fgt * cold + ig * Tanh(zc);
            hn = Sigmoid(zo + p[1][i] * cn) * Tanh(cn);
            c[j][i] = valid ? cn : cold;
          } else {
            const float zg = Sigmoid(Clip(acc[0][i] + xw[0][i], clip));
            const float rg = Sigmoid(Clip(acc[1][i] + xw[1][i], clip));
            const float hh = Tanh(Clip(xw[2][i] + rg * (acc[2][i] + p[0][i]), clip));
            hn = (1.0f - zg) * hh + zg * hold[i];
          }
          hout[i] = valid ? hn : hold[i];
          yv[i] = valid ? hn : 0.f;
        }
        *reinterpret_cast<f4*>(hnxt + fr * pitch + col) = hout;
        if (live) store4(yrow, col, yv);
      }
    }
    __syncthreads();
  }

  const float* const hfin = CELL == 2 ? hb0 : ((T & 1) ? hb1 : hb0);
  if (live) {
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int u = wid + j * NW, col = col0 + j * NW * 16;
      if (u >= KC) break;
      store4(a.yh + sbase + static_cast<int64_t>(n) * H, col, *reinterpret_cast<const f4*>(hfin + fr * pitch + col));
      if (CELL == 0 && a.yc) store4(a.yc + sbase + static_cast<int64_t>(n) * H, col, c[j]);
    }
  }
}

template <int CELL, int TPW>
int Launch(const RnnArgs& a, int Hp, int NW, size_t lds, hipStream_t st) {
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&rnn_kernel<CELL, TPW>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess)
    return -3;
  hipLaunchKernelGGL((rnn_kernel<CELL, TPW>), dim3((a.N + 15) / 16, a.nd), dim3(NW * 64), lds, st, a, Hp, NW);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <int CELL>
int LaunchCell(const RnnArgs& a, int Hp, hipStream_t st) {
  const int NT = Hp / 16, tpw = NT <= kMaxWaves ? 1 : 4;
  const int NW = (NT + tpw - 1) / tpw;
  const size_t lds = static_cast<size_t>(2) * 16 * (Hp + kPad) * sizeof(float);
  if (tpw == 1) return Launch<CELL, 1>(a, Hp, NW, lds, st);
  return Launch<CELL, 4>(a, Hp, NW, lds, st);
}

}  // namespace

int RnnMfma(const RnnArgs& a, void* stream) {
  if (!a.xw || !a.r || !a.y || !a.yh || (a.cell != 0 && a.cell != 1)) return -2;
  // not taken (the caller keeps its own path)
  if (a.T < 1 || a.N < 1 || a.H < 1 || a.H > kMaxHidden || a.nd < 1 || a.nd > 2) return -4;
  if (a.N > 16 * 65535 || !(a.clip >= 0.f)) return -4;
  for (const void* p : {static_cast<const void*>(a.xw), static_cast<const void*>(a.r),
                        static_cast<const void*>(a.peep), static_cast<const void*>(a.rbh)})
    if (reinterpret_cast<uintptr_t>(p) % 16) return -4;
  if (a.H % 4 == 0)
    for (const void* p :
         {static_cast<const void*>(a.y), static_cast<const void*>(a.yh), static_cast<const void*>(a.yc)})
      if (reinterpret_cast<uintptr_t>(p) % 16) return -4;
  const int Hp = (a.H + 15) & ~15;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.cell == 0) return LaunchCell<0>(a, Hp, st);
  return a.linear_before_reset ? LaunchCell<1>(a, Hp, st) : LaunchCell<2>(a, Hp, st);
}

}  // namespace smlnn
