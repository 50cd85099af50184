// K27: one ALS half-sweep on gfx950: for every row r of one side, gather the other side's factor rows of what r
// rated, build the k x k normal equations on fp64 matrix instructions and solve them by Cholesky.
//
//   explicit:  A_r = sum_c y_c y_c^T + lam max(n_r, 1) I          b_r = sum_c val_c y_c
//   implicit:  A_r = YtY + sum_c (alpha val_c) y_c y_c^T + lam I   b_r = sum_{c: val_c > 0} (1 + alpha val_c) y_c
//
// Factors are fp64 [n, kp] with kp = rank padded to 16 / 32 / 48 / 64 and zero pad columns, so a factor row is
// kp / 16 aligned 128-byte pieces. The host (ops/als.py) turns the CSR into tasks, longest first: a task is
// (row, first nonzero, length <= L, slot). Rows longer than L are cut into segments with consecutive workspace
// slots; every other task has slot -1.
//
// Sweep kernel: one wave per task, no block-level barrier; wave g of the persistent grid takes tasks g, g + G,
// ... A step feeds 4 nonzeros to v_mfma_f64_16x16x4_f64: lane l gathers, for nonzero l / 16 of the step, column
// 16 t + l % 16 of its factor row for every 16-column piece t, straight from global memory into registers. These
// registers are the B operand and, scaled by the nonzero's weight, the A operand; only the tiles (ti <= tj) of
// the upper triangle are accumulated (10 tiles, 80 accumulator registers at kp = 64). Gathers are double
// buffered in registers: the next chunk of steps is in flight while the current one multiplies. b is summed on
// the VALU from the same registers, per lane, and folded over the 4 nonzero slots once per task. Steps past the
// end of a task feed zeros.
//   A task with slot -1 moves (A, b) into its wave's odd-pitch LDS tile, adds the diagonal (and YtY), runs a
// right-looking Cholesky over the leading k columns, substitutes forward and back with b in one register per
// lane, and writes X[row]. A pivot that is not a finite positive number makes the row NaN; every loop is
// bounded by k. A task with a slot stores its partial (A, b) to the [slots, kp kp + kp] workspace instead.
// Reduce kernel: one wave per cut row sums the row's slots in index order and runs the same solve. YtY uses the
// same pair: the "row" is all of Y with weight 1, cut every L rows, and the reduce kernel stores the sum. No
// atomics anywhere: results do not depend on scheduling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "nn_ops.h"

namespace smlnn {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;  // waves (independent rows) per block

struct SweepArgs {
  const int32_t* indices;  // null: the gram pass over all of Y
  const double* val;
  const int64_t* tasks;    // [ntasks, 4] row, first nonzero, length, slot
  const int64_t* red;      // [nred, 4] row, first slot, slots, n_r
  const double* Y;
  double* X;
  const double* yty;       // [kp, kp], implicit only
  double* ws;              // [slots, kp kp + kp]
  double* gram_out;        // reduce kernel, gram pass: where the sum goes
  int64_t ntasks, nred, nY;
  int k, kp, L;
  int implicit, nonneg, gram;
  double lam, alpha;
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// v of lane `lane` (the same lane for the whole wave)
__device__ __forceinline__ double read_lane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// steps per gather chunk: two chunks of kSteps * KT doubles per lane are live
template <int KT>
struct Tiling {
  static constexpr int kSteps = KT == 1 ? 8 : KT == 2 ? 4 : 2;
  static constexpr int kTiles = KT * (KT + 1) / 2;
};

template <int KT>
struct Chunk {
  double y[Tiling<KT>::kSteps][KT];
  double wa[Tiling<KT>::kSteps], wb[Tiling<KT>::kSteps];
};

// gathers of steps s0 .. s0 + kSteps of a task: this lane's nonzero of each step and its KT columns
template <int KT>
__device__ __forceinline__ void gather(Chunk<KT>& c, const SweepArgs& a, int64_t beg, int len, int s0, int lane) {
#pragma unroll
  for (int u = 0; u < Tiling<KT>::kSteps; ++u) {
    const int e = 4 * (s0 + u) + (lane >> 4);
    double wa = 0.0, wb = 0.0;
    int64_t src = -1;
    if (e < len) {
      if (a.gram) {
        src = beg + e;
        wa = 1.0;
      } else {
        src = a.indices[beg + e];
        const double v = a.val[beg + e];
        wa = a.implicit ? a.alpha * v : 1.0;
        wb = a.implicit ? (v > 0.0 ? 1.0 + a.alpha * v : 0.0) : v;
      }
    }
    c.wa[u] = wa;
    c.wb[u] = wb;
#pragma unroll
    for (int t = 0; t < KT; ++t) c.y[u][t] = src >= 0 ? a.Y[src * a.kp + 16 * t + (lane & 15)] : 0.0;
  }
}

template <int KT>
__device__ __forceinline__ void multiply(const Chunk<KT>& c, d4 (&acc)[Tiling<KT>::kTiles], double (&b)[KT]) {
#pragma unroll
  for (int u = 0; u < Tiling<KT>::kSteps; ++u) {
    double ya[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      ya[t] = c.wa[u] * c.y[u][t];
      b[t] = fma(c.wb[u], c.y[u][t], b[t]);
    }
    int tile = 0;
#pragma unroll
    for (int ti = 0; ti < KT; ++ti)
#pragma unroll
      for (int tj = ti; tj < KT; ++tj, ++tile)
        acc[tile] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[ti], c.y[u][tj], acc[tile], 0, 0, 0);
  }
}

// (A, b) of a task out of the registers, A in full (both triangles) at the given pitch. Result register v of
// tile (ti, tj) is element (16 ti + 4 v + lane / 16, 16 tj + lane % 16); after the fold lanes 0-15 hold b.
template <int KT>
__device__ __forceinline__ void store_system(const d4 (&acc)[Tiling<KT>::kTiles], const double (&b)[KT], double* dst,
                                             int pitch, double* bdst, int lane) {
  int tl = 0;
#pragma unroll
  for (int ti = 0; ti < KT; ++ti)
#pragma unroll
    for (int tj = ti; tj < KT; ++tj, ++tl)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = 16 * ti + 4 * v + (lane >> 4), j = 16 * tj + (lane & 15);
        dst[i * pitch + j] = acc[tl][v];
        if (ti != tj) dst[j * pitch + i] = acc[tl][v];
      }
  if (lane < 16)
#pragma unroll
    for (int t = 0; t < KT; ++t) bdst[16 * t + lane] = b[t];
}

// Cholesky solve of the wave's LDS system: tile [kp][kp + 1] (lower triangle read), bl [kp]. Writes x [kp]:
// the solution in the leading k columns, zeros in the pad.
__device__ void solve_row(double* tile, double* bl, const SweepArgs& a, double diag, double* x, int lane) {
  const int k = a.k, P = a.kp + 1;
  if (a.implicit)
    for (int i = 0; i < k; ++i)
      if (lane < k) tile[i * P + lane] += a.yty[i * a.kp + lane];
  if (lane < k) tile[lane * P + lane] += diag;
  wave_sync();
  bool bad = false;
  double r_own = 1.0;  // lane i: L[i][i]
  for (int c = 0; c < k; ++c) {
    const double d = tile[c * P + c];
    bad |= !(d > 0.0 && d < std::numeric_limits<double>::infinity());
    const double r = sqrt(d);
    double l = 0.0;
    if (lane == c) r_own = r;
    if (lane > c && lane < k) {
      l = tile[lane * P + c] / r;
      tile[lane * P + c] = l;
    }
    for (int j = c + 1; j < k; ++j) {
      const double lj = read_lane(l, j);
      if (lane >= j && lane < k) tile[lane * P + j] -= l * lj;
    }
    wave_sync();
  }
  double v = lane < k ? bl[lane] : 0.0;
  for (int c = 0; c < k; ++c) {  // L z = b
    const double z = read_lane(v, c) / read_lane(r_own, c);
    if (lane == c) v = z;
    if (lane > c && lane < k) v -= tile[lane * P + c] * z;
  }
  for (int c = k - 1; c >= 0; --c) {  // L^T x = z
    const double z = read_lane(v, c) / read_lane(r_own, c);
    if (lane == c) v = z;
    if (lane < c) v -= tile[c * P + lane] * z;
  }
  if (bad) v = std::numeric_limits<double>::quiet_NaN();
  if (a.nonneg && v < 0.0) v = 0.0;
  if (lane < a.kp) x[lane] = lane < k ? v : 0.0;
}

template <int KT>
__global__ __launch_bounds__(kWaves * 64) void als_sweep_kernel(const SweepArgs a) {
  extern __shared__ double lds[];
  constexpr int KP = 16 * KT, P = KP + 1, NT = Tiling<KT>::kTiles, U = Tiling<KT>::kSteps;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* tile = lds + wave * (KP * P + KP);
  double* bl = tile + KP * P;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kWaves;
  for (int64_t task = static_cast<int64_t>(blockIdx.x) * kWaves + wave; task < a.ntasks; task += stride) {
    int64_t row, beg, slot;
    int len;
    if (a.gram) {
      row = 0; beg = task * a.L; slot = task;
      len = static_cast<int>(std::min<int64_t>(a.L, a.nY - beg));
    } else {
      const int64_t* t = a.tasks + 4 * task;
      row = t[0]; beg = t[1]; len = static_cast<int>(t[2]); slot = t[3];
    }
    d4 acc[NT];
    double b[KT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < KT; ++t) b[t] = 0.0;
    const int chunks = ((len + 3) / 4 + U - 1) / U;
    Chunk<KT> c0, c1;
    if (chunks > 0) gather<KT>(c0, a, beg, len, 0, lane);
    for (int c = 0; c < chunks; c += 2) {
      if (c + 1 < chunks) gather<KT>(c1, a, beg, len, (c + 1) * U, lane);
      multiply<KT>(c0, acc, b);
      if (c + 1 < chunks) {
        if (c + 2 < chunks) gather<KT>(c0, a, beg, len, (c + 2) * U, lane);
        multiply<KT>(c1, acc, b);
      }
    }
#pragma unroll
    for (int t = 0; t < KT; ++t) {  // fold the 4 nonzero slots; lanes 0-15 hold column 16 t + lane
      b[t] += __shfl_xor(b[t], 16);
      b[t] += __shfl_xor(b[t], 32);
    }
    if (slot >= 0) {
      double* dst = a.ws + slot * (KP * KP + KP);
      store_system<KT>(acc, b, dst, KP, dst + KP * KP, lane);
    } else {
      store_system<KT>(acc, b, tile, P, bl, lane);
    }
    if (slot < 0) {
      wave_sync();
      const double diag = a.implicit ? a.lam : a.lam * static_cast<double>(std::max(len, 1));
      solve_row(tile, bl, a, diag, a.X + row * KP, lane);
      wave_sync();  // the tile is reused by the wave's next task
    }
  }
}

// one wave per cut row: the sum of its slots in index order, then the solve (or, gram pass, the store)
__global__ __launch_bounds__(kWaves * 64) void als_reduce_kernel(const SweepArgs a) {
  extern __shared__ double lds[];
  const int kp = a.kp, P = kp + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* tile = lds + wave * (kp * P + kp);
  double* bl = tile + kp * P;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (r >= a.nred) return;
  const int64_t row = a.gram ? 0 : a.red[4 * r], slot0 = a.gram ? 0 : a.red[4 * r + 1];
  const int64_t slots = a.gram ? (a.nY + a.L - 1) / a.L : a.red[4 * r + 2];
  const int per = kp * kp + kp;
  for (int e = lane; e < per; e += 64) {
    double s = 0.0;
    for (int64_t g = 0; g < slots; ++g) s += a.ws[(slot0 + g) * per + e];
    if (a.gram) {
      if (e < kp * kp) a.gram_out[e] = s;
    } else if (e < kp * kp) {
      tile[(e / kp) * P + e % kp] = s;
    } else {
      bl[e - kp * kp] = s;
    }
  }
  if (a.gram) return;
  wave_sync();
  const double diag = a.implicit ? a.lam : a.lam * static_cast<double>(std::max<int64_t>(a.red[4 * r + 3], 1));
  solve_row(tile, bl, a, diag, a.X + row * kp, lane);
}

int cu_count() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) {
    (void)hipGetLastError();
    v = 256;
  }
  return v;
}

size_t lds_bytes(int kp) { return static_cast<size_t>(kWaves) * (kp * (kp + 1) + kp) * sizeof(double); }

template <typename K>
int prepare_kernel(K kernel, size_t lds) {
  if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds)) != hipSuccess)
    return -3;
  return 0;
}

// the persistent sweep grid for `tasks` tasks, then the reduce grid for a.nred rows
template <int KT>
int launch_pair(const SweepArgs& a, hipStream_t s) {
  const size_t lds = lds_bytes(16 * KT);
  if (prepare_kernel(als_sweep_kernel<KT>, lds) != 0 || prepare_kernel(als_reduce_kernel, lds) != 0) return -3;
  if (a.ntasks > 0) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, als_sweep_kernel<KT>, kWaves * 64, lds) != hipSuccess ||
        per_cu < 1) {
      (void)hipGetLastError();
      per_cu = 1;
    }
    const int64_t grid = std::min<int64_t>((a.ntasks + kWaves - 1) / kWaves, static_cast<int64_t>(per_cu) * cu_count());
    hipLaunchKernelGGL(als_sweep_kernel<KT>, dim3(static_cast<unsigned>(grid)), dim3(kWaves * 64), lds, s, a);
  }
  if (a.nred > 0)
    hipLaunchKernelGGL(als_reduce_kernel, dim3(static_cast<unsigned>((a.nred + kWaves - 1) / kWaves)),
                       dim3(kWaves * 64), lds, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_kt(const SweepArgs& a, hipStream_t s) {
  switch (a.kp / 16) {
    case 1: return launch_pair<1>(a, s);
    case 2: return launch_pair<2>(a, s);
    case 3: return launch_pair<3>(a, s);
    default: return launch_pair<4>(a, s);
  }
}

}  // namespace

int AlsSweep(const AlsArgs& f, void* stream) {
  if (!f.indices || !f.val || !f.tasks || !f.Y || !f.X || f.nX <= 0 || f.nY <= 0 || f.ntasks < 0 || f.nred < 0 ||
      f.slots < 0 || f.seg_len < 4)
    return -4;
  if (f.k < 1 || f.k > kAlsMaxRank || f.kp != (f.k + 15) / 16 * 16 || !(f.lam > 0.0) || !std::isfinite(f.lam) ||
      !std::isfinite(f.alpha))
    return -4;
  if ((f.nred > 0 && !f.red) || (f.nred > 0) != (f.slots > 0) || f.ntasks > INT32_MAX * static_cast<int64_t>(kWaves) ||
      f.nred > INT32_MAX * static_cast<int64_t>(kWaves))
    return -4;
  const int64_t per = static_cast<int64_t>(f.kp) * f.kp + f.kp;
  const int64_t gram_slots = f.implicit ? (f.nY + f.seg_len - 1) / f.seg_len : 0;
  if (std::max(f.slots, gram_slots) > 0 && (!f.ws || f.ws_doubles / per < std::max(f.slots, gram_slots))) return -4;
  if (f.implicit && !f.yty) return -4;
  hipStream_t s = static_cast<hipStream_t>(stream);
  SweepArgs a;
  a.indices = f.indices; a.val = f.val; a.tasks = f.tasks; a.red = f.red; a.Y = f.Y; a.X = f.X;
  a.yty = f.yty; a.ws = f.ws; a.gram_out = nullptr;
  a.ntasks = f.ntasks; a.nred = f.nred; a.nY = f.nY;
  a.k = f.k; a.kp = f.kp; a.L = f.seg_len;
  a.implicit = f.implicit; a.nonneg = f.nonnegative; a.gram = 0;
  a.lam = f.lam; a.alpha = f.alpha;
  if (f.implicit) {  // YtY first: all of Y with weight 1, cut every seg_len rows, summed by the reduce kernel
    SweepArgs g = a;
    g.indices = nullptr; g.val = nullptr; g.tasks = nullptr; g.red = nullptr; g.X = nullptr; g.yty = nullptr;
    g.gram = 1; g.implicit = 0; g.ntasks = gram_slots; g.nred = 1; g.gram_out = f.yty;
    const int rc = launch_kt(g, s);
    if (rc != 0) return rc;
  }
  return launch_kt(a, s);
}

}  // namespace smlnn
