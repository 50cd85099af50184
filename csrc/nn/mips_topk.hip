// K23: fused top-k maximum-inner-product search on the CDNA4 fp32 matrix cores (module _nn; the device path
// of KNN / ConditionalKNN).
//
//   for every query m: the k largest q[m, :] . keys[n, :] over the eligible keys n, descending, ties by the
//   smaller n; key n is eligible iff bit key_label[n] of allow[m] is set (no conditioner: every key)
//
// The [M, N] score matrix never exists in memory: scores live in MFMA accumulators, are compared against the
// query's current k-th best in registers, and only the few that pass reach LDS.
//
// Work split: grid (query tiles of 64, key splits); 256 threads = 4 waves. A block streams its contiguous key
// range in tiles of 128 keys; wave w owns keys 32 w .. 32 w + 31 of the tile against all 64 queries: 2 x 4
// accumulator blocks of v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation). Keys are the first
// MFMA operand, queries the second, so a lane holds keys 4 (lane / 16) + 0..3 of each 16-key block for the one
// query lane % 16 of each 16-query block: every threshold compare is register-local.
//
// Staging: D is looped in chunks of 32 floats. A chunk of the key tile (128 rows) and of the query tile (64
// rows) is staged in LDS at a row pitch of 160 bytes (an odd multiple of 32 bytes: conflict-free for the
// 16-lane ds_read_b128, as conv_mfma / attn_mfma measured), double-buffered: the 16-byte buffer loads of step
// s + 1 are issued before the MFMAs of step s and written to the other buffer after them, one barrier per
// step. Rows past N or M read as zero through the buffer resource; columns past D are zeroed in registers
// (a row pitch wider than D may hold anything). The key buffer resource is rebased per tile with 64-bit
// arithmetic, so N * pitch * 4 may pass 4 GiB while in-tile offsets stay 32-bit. One ds_read_b128 of a lane
// feeds four consecutive MFMAs: MFMA (h, i) of a chunk has lane group g multiply column 16 h + 4 g + i, the
// same permutation for both operands. A last chunk of at most 16 columns runs only its h = 0 half.
//
// Selection: a candidate is one uint64, the order-preserving map of the fp32 score (-0.0 as +0.0) in the high
// word and ~index in the low word: a larger integer is a better candidate, ties included. 0 is the empty slot
// (it decodes to -inf / -1). Per query LDS holds the sorted best list (KCAP entries), a pending buffer (KCAP
// entries) with an atomic fill count, and the threshold (the k-th best), which every lane also keeps in
// registers for its four queries, as a float for the first filter. After a key tile a lane compares its 32
// scores with the float thresholds; a wave with an empty ballot does nothing more for the tile. A passing
// score is packed, compared exactly, has its conditioner bit tested (the tile's labels and the query tile's
// allow words are in LDS) and is appended to the pending buffer by an LDS atomic. An append that finds the
// buffer full keeps its candidate in the lane; one __syncthreads_or per tile decides uniformly whether to
// merge (a buffer at least half full, or a failed append), after which the failed appends are retried against
// the raised thresholds, as often as needed: no candidate is ever dropped, whatever the key order. The merge
// is one wave per query, 16 queries per wave: bitonic sort of the pending entries ascending across lanes,
// element-wise max with the descending best list (the top KCAP of the union, a bitonic sequence), bitonic
// merge back to descending.
//
// Key splits: with fewer query tiles than the device holds blocks, gridDim.y blocks share the keys of a query
// tile; each writes its sorted list of packed candidates to ws[split][M][k], and mips_reduce_kernel (one wave
// per query) merges them in the same order. With one split the main kernel writes vals / idx itself.
//
// Tiles: 64 queries x 128 keys x 32 floats. LDS: 60 KiB staging + 2 x 64 x KCAP x 8 lists + 16 KiB of allow
// words (conditioner forms only): 77 KiB for KCAP 16 (two blocks per CU), 94 KiB with the conditioner, 125 /
// 142 KiB for KCAP 64 (one block per CU). No scratch in any form.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nn_ops.h"

namespace smlnn {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kBQ = 64, kBK = 128, kBD = 32;  // queries per block, keys per tile, floats per chunk
constexpr int kPitch = 160;                   // LDS row pitch in bytes (32 floats + 32 bytes)
constexpr int kKStage = kBK * kPitch, kStage = (kBK + kBQ) * kPitch;
constexpr int kMaxW = kMipsMaxLabels / 32;    // allow words per query
constexpr uint32_t kOob = 0x80000000u;        // past every buffer resource's range: the load returns zero

__device__ __forceinline__ uint4 Load16(__amdgpu_buffer_rsrc_t rsrc, uint32_t off) {
  auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
  uint4 r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}

// fp32 -> uint32 with the same order (finite values and infinities); -0.0 maps like +0.0
__device__ __forceinline__ uint32_t Mono(float s) {
  uint32_t b = __float_as_uint(s);
  if (b == 0x80000000u) b = 0;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float UnMono(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}
__device__ __forceinline__ uint64_t Pack(float s, int idx) {
  return (static_cast<uint64_t>(Mono(s)) << 32) | static_cast<uint32_t>(~idx);
}
// the float a score must reach to be worth packing: -inf for the empty slot, NaN (nothing passes) for ~0
__device__ __forceinline__ float ThrFloat(uint64_t t) {
  return t == 0 ? -__builtin_inff() : UnMono(static_cast<uint32_t>(t >> 32));
}
__device__ __forceinline__ uint64_t Max64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t Min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// a bitonic sequence over lanes [0, W) of every W-lane group -> descending
template <int W>
__device__ __forceinline__ uint64_t BitonicMergeDesc(uint64_t e, int lane) {
#pragma unroll
  for (int j = W / 2; j > 0; j >>= 1) {
    const uint64_t o = __shfl_xor(e, j);
    e = (lane & j) == 0 ? Max64(e, o) : Min64(e, o);
  }
  return e;
}
// any values -> ascending within every W-lane group
template <int W>
__device__ __forceinline__ uint64_t BitonicSortAsc(uint64_t e, int lane) {
#pragma unroll
  for (int k = 2; k <= W; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint64_t o = __shfl_xor(e, j);
      const bool up = (lane & k) == 0 || k == W, lower = (lane & j) == 0;
      e = lower == up ? Min64(e, o) : Max64(e, o);
    }
  return e;
}

template <int KCAP, bool COND>
__global__ __launch_bounds__(kThreads) void mips_topk_kernel(MipsArgs a, int tiles_per_split) {
  constexpr int P = KCAP, HALF = KCAP / 2;  // pending slots per query; fill at which a merge is asked for
  __shared__ __attribute__((aligned(16))) uint8_t stage[2 * kStage];
  __shared__ uint64_t best[kBQ * KCAP];
  __shared__ uint64_t pend[kBQ * P];
  __shared__ uint64_t thr_s[kBQ];
  __shared__ uint32_t cnt[kBQ];
  __shared__ int lab[COND ? 2 * kBK : 1];
  __shared__ uint32_t allow_s[COND ? kBQ * kMaxW : 1];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int q0 = blockIdx.x * kBQ;
  const int M = a.M, N = a.N, D = a.D, k = a.k, W = a.W;
  const int NC = (D + kBD - 1) / kBD;
  const int total_tiles = (N + kBK - 1) / kBK;
  const int t_begin = static_cast<int>(blockIdx.y) * tiles_per_split;
  const int t_end = t_begin + tiles_per_split < total_tiles ? t_begin + tiles_per_split : total_tiles;
  const int64_t nsteps = t_end > t_begin ? static_cast<int64_t>(t_end - t_begin) * NC : 0;

  for (int i = tid; i < kBQ * KCAP; i += kThreads) best[i] = 0;
  if (tid < kBQ) {
    cnt[tid] = 0;
    thr_s[tid] = q0 + tid < M ? 0ull : ~0ull;  // rows past M take no candidate
  }
  if constexpr (COND) {
    for (int i = tid; i < kBQ * W; i += kThreads) {
      const int q = i / W, w = i - q * W;
      allow_s[q * kMaxW + w] = q0 + q < M ? a.allow[static_cast<int64_t>(q0 + q) * W + w] : 0u;
    }
  }

  // query rows of the block: one resource; key rows: one per tile
  const int qrows = M - q0 < kBQ ? M - q0 : kBQ;
  const int D4 = (D + 3) & ~3;
  const uint32_t qpb = static_cast<uint32_t>(a.q_pitch) * 4, kpb = static_cast<uint32_t>(a.k_pitch) * 4;
  const auto rq = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.q + static_cast<int64_t>(q0) * a.q_pitch), 0,
      static_cast<int>(((qrows - 1) * a.q_pitch + D4) * 4), 0x00020000);

  uint4 kreg[4], qreg[2];
  int labreg = -1;
  auto mask_cols = [&](uint4 v, int col) {
    const int rem = D - col;  // columns of this 16-byte piece inside D
    if (rem < 4) {
      if (rem < 1) v.x = 0;
      if (rem < 2) v.y = 0;
      if (rem < 3) v.z = 0;
      v.w = 0;
    }
    return v;
  };
  auto load_step = [&](int t, int c) {
    const int k0 = t * kBK;
    const int krows = N - k0 < kBK ? N - k0 : kBK;
    const auto rk = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.keys + static_cast<int64_t>(k0) * a.k_pitch), 0,
        static_cast<int>(((krows - 1) * a.k_pitch + D4) * 4), 0x00020000);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + kThreads * i, row = e >> 3, col = c * kBD + (e & 7) * 4;
      kreg[i] = mask_cols(Load16(rk, row < krows && col < D ? row * kpb + col * 4 : kOob), col);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + kThreads * i, row = e >> 3, col = c * kBD + (e & 7) * 4;
      qreg[i] = mask_cols(Load16(rq, row < qrows && col < D ? row * qpb + col * 4 : kOob), col);
    }
    if constexpr (COND) {
      if (c == 0 && tid < kBK) labreg = k0 + tid < N ? a.key_label[k0 + tid] : -1;
    }
  };
  auto store_step = [&](int buf, int t, int c) {
    uint8_t* s = stage + buf * kStage;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + kThreads * i;
      *reinterpret_cast<uint4*>(s + (e >> 3) * kPitch + (e & 7) * 16) = kreg[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + kThreads * i;
      *reinterpret_cast<uint4*>(s + kKStage + (e >> 3) * kPitch + (e & 7) * 16) = qreg[i];
    }
    if constexpr (COND) {
      if (c == 0 && tid < kBK) lab[(t & 1) * kBK + tid] = labreg;
    }
  };

  f4 acc[2][4];
  auto clear_acc = [&]() {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int qs = 0; qs < 4; ++qs) acc[ks][qs] = f4{0.f, 0.f, 0.f, 0.f};
  };
  auto compute = [&](int buf, int c) {
    const bool both = D - c * kBD > 16;  // the chunk's second 16 columns hold data
    const uint8_t* s = stage + buf * kStage;
    f4 af[2][2], bf[4][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        af[ks][h] = *reinterpret_cast<const f4*>(s + (wid * 32 + ks * 16 + fr) * kPitch + h * 64 + fg * 16);
#pragma unroll
      for (int qs = 0; qs < 4; ++qs)
        bf[qs][h] = *reinterpret_cast<const f4*>(s + kKStage + (qs * 16 + fr) * kPitch + h * 64 + fg * 16);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (h == 1 && !both) break;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int qs = 0; qs < 4; ++qs)
            acc[ks][qs] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ks][h][i], bf[qs][h][i], acc[ks][qs], 0, 0, 0);
    }
  };

  // thresholds of this lane's four queries (16 qs + fr)
  uint64_t thr[4];
  float thrf[4];
  auto load_thr = [&]() {
#pragma unroll
    for (int qs = 0; qs < 4; ++qs) {
      thr[qs] = thr_s[qs * 16 + fr];
      thrf[qs] = ThrFloat(thr[qs]);
    }
  };
  // all waves: fold every query's pending entries into its best list, raise the thresholds
  auto merge = [&]() {
    for (int i = 0; i < 16; ++i) {
      const int q = wid * 16 + i;
      uint32_t c = cnt[q];
      if (c == 0) continue;
      c = c < P ? c : P;
      const uint64_t e0 = lane < KCAP ? best[q * KCAP + lane] : 0ull;
      uint64_t e1 = lane < static_cast<int>(c) ? pend[q * P + lane] : 0ull;
      e1 = BitonicSortAsc<KCAP>(e1, lane);
      const uint64_t e = BitonicMergeDesc<KCAP>(Max64(e0, e1), lane);
      if (lane < KCAP) best[q * KCAP + lane] = e;
      if (lane == k - 1) thr_s[q] = e;
      if (lane == 0) cnt[q] = 0;
    }
    __syncthreads();
    load_thr();
  };
  // after the last chunk of key tile t: scores against thresholds, appends, merges as needed
  auto select = [&](int t) {
    const int k0 = t * kBK, kin0 = wid * 32 + fg * 4;
    uint32_t mask = 0;
#pragma unroll
    for (int qs = 0; qs < 4; ++qs)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (acc[ks][qs][r] >= thrf[qs]) mask |= 1u << ((qs * 2 + ks) * 4 + r);
    if (k0 + kBK > N) {  // rows past N were read as zero
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (k0 + kin0 + ks * 16 + r >= N) mask &= ~(0x01010101u << (ks * 4 + r));
    }
    for (;;) {
      int want = 0;
      if (__any(mask != 0)) {
#pragma unroll
        for (int qs = 0; qs < 4; ++qs)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const uint32_t bit = 1u << ((qs * 2 + ks) * 4 + r);
              if (mask & bit) {
                const int kin = kin0 + ks * 16 + r, ql = qs * 16 + fr;
                const uint64_t key = Pack(acc[ks][qs][r], k0 + kin);
                bool ok = key > thr[qs];
                if constexpr (COND) {
                  if (ok) {
                    const uint32_t l = static_cast<uint32_t>(lab[(t & 1) * kBK + kin]);
                    ok = l < static_cast<uint32_t>(W) * 32u && ((allow_s[ql * kMaxW + (l >> 5)] >> (l & 31)) & 1u);
                  }
                }
                if (!ok) {
                  mask &= ~bit;
                } else {
                  const uint32_t slot = atomicAdd(&cnt[ql], 1u);
                  if (slot < P) {
                    pend[ql * P + slot] = key;
                    mask &= ~bit;
                  }
                  if (slot + 1 >= HALF) want = 1;
                }
              }
            }
      }
      if (!__syncthreads_or(want)) break;
      merge();
    }
  };

  clear_acc();
  if (nsteps > 0) {
    load_step(t_begin, 0);
    store_step(0, t_begin, 0);
  }
  __syncthreads();
  load_thr();
  int ct = t_begin, cc = 0;  // the step being computed
  for (int64_t s = 0; s < nsteps; ++s) {
    const int buf = static_cast<int>(s & 1);
    int nt = ct, nc = cc + 1;
    if (nc == NC) {
      nc = 0;
      ++nt;
    }
    const bool more = s + 1 < nsteps;
    if (more) load_step(nt, nc);
    compute(buf, cc);
    if (nc == 0) {
      select(ct);
      clear_acc();
    }
    if (more) store_step(buf ^ 1, nt, nc);
    __syncthreads();
    ct = nt;
    cc = nc;
  }
  merge();  // what is still pending

  for (int i = tid; i < kBQ * k; i += kThreads) {
    const int q = i / k, j = i - q * k, m = q0 + q;
    if (m >= M) continue;
    const uint64_t e = best[q * KCAP + j];
    if (a.splits > 1) {
      a.ws[(static_cast<int64_t>(blockIdx.y) * M + m) * k + j] = e;
    } else {
      a.vals[static_cast<int64_t>(m) * k + j] = ThrFloat(e);
      a.idx[static_cast<int64_t>(m) * k + j] = static_cast<int32_t>(~static_cast<uint32_t>(e));
    }
  }
}

// one wave per query: the splits' descending lists -> vals / idx
__global__ __launch_bounds__(kThreads) void mips_reduce_kernel(MipsArgs a) {
  const int lane = threadIdx.x & 63, m = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (m >= a.M) return;
  const int k = a.k;
  uint64_t e = lane < k ? a.ws[static_cast<int64_t>(m) * k + lane] : 0ull;
  for (int s = 1; s < a.splits; ++s) {
    const int r = 63 - lane;  // the other list ascending
    const uint64_t o = r < k ? a.ws[(static_cast<int64_t>(s) * a.M + m) * k + r] : 0ull;
    e = BitonicMergeDesc<64>(Max64(e, o), lane);
  }
  if (lane < k) {
    a.vals[static_cast<int64_t>(m) * k + lane] = ThrFloat(e);
    a.idx[static_cast<int64_t>(m) * k + lane] = static_cast<int32_t>(~static_cast<uint32_t>(e));
  }
}

int CuCount() {
  static int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return 0;
    return n;
  }();
  return cus;
}

}  // namespace

int MipsSplitPlan(int M, int N, int k, int conditioned) {
  if (M <= 0 || N <= 0) return 1;
  const int64_t qt = (static_cast<int64_t>(M) + kBQ - 1) / kBQ, tiles = (static_cast<int64_t>(N) + kBK - 1) / kBK;
  const int64_t slots = static_cast<int64_t>(CuCount()) * (k <= 16 && !conditioned ? 2 : 1);  // resident blocks
  int64_t s = slots / qt;
  const int64_t by_work = (tiles + 7) / 8;  // a split streams at least 8 key tiles
  if (s > by_work) s = by_work;
  if (s > 1024) s = 1024;
  return s < 1 ? 1 : static_cast<int>(s);
}

int MipsTopk(const MipsArgs& in, void* stream) {
  MipsArgs a = in;
  if (a.M <= 0) return 0;
  if (!a.q || !a.keys || !a.vals || !a.idx || a.N <= 0 || a.D <= 0 || a.k <= 0) return -2;
  if ((a.key_label == nullptr) != (a.allow == nullptr)) return -2;
  const bool cond = a.key_label != nullptr;
  // not taken (the caller keeps its own path)
  if (a.k > 64 || (cond && (a.W < 1 || a.W > kMaxW))) return -4;
  const int64_t d4 = (static_cast<int64_t>(a.D) + 3) & ~3ll;
  if (a.N > INT32_MAX - 255) return -4;
  // 32-bit byte offsets inside one tile of 128 rows
  if (a.q_pitch < d4 || a.k_pitch < d4 || a.q_pitch % 4 || a.k_pitch % 4 || a.k_pitch > (1 << 21) ||
      a.q_pitch > (1 << 21))
    return -4;
  if (reinterpret_cast<uintptr_t>(a.q) % 16 || reinterpret_cast<uintptr_t>(a.keys) % 16) return -4;
  const int tiles = (a.N + kBK - 1) / kBK;
  if (a.splits <= 0) a.splits = MipsSplitPlan(a.M, a.N, a.k, cond);
  if (a.splits > tiles) a.splits = tiles;
  if (a.splits > 65535) a.splits = 65535;
  if (a.splits > 1 && !a.ws) return -2;
  const int tps = (tiles + a.splits - 1) / a.splits;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((a.M + kBQ - 1) / kBQ, a.splits);
  if (a.k <= 16) {
    if (cond) hipLaunchKernelGGL((mips_topk_kernel<16, true>), grid, dim3(kThreads), 0, st, a, tps);
    else hipLaunchKernelGGL((mips_topk_kernel<16, false>), grid, dim3(kThreads), 0, st, a, tps);
  } else {
    if (cond) hipLaunchKernelGGL((mips_topk_kernel<64, true>), grid, dim3(kThreads), 0, st, a, tps);
    else hipLaunchKernelGGL((mips_topk_kernel<64, false>), grid, dim3(kThreads), 0, st, a, tps);
  }
  if (hipGetLastError() != hipSuccess) return -3;
  if (a.splits > 1) {
    hipLaunchKernelGGL(mips_reduce_kernel, dim3((a.M + 3) / 4), dim3(kThreads), 0, st, a);
    if (hipGetLastError() != hipSuccess) return -3;
  }
  return 0;
}

}  // namespace smlnn
