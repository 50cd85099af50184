// K26: fused forest walk for the ai.onnx.ml TreeEnsembleClassifier / TreeEnsembleRegressor operators on gfx950.
//
// Packed forest (built on the host by ops/trees.py). One 16-byte record per node, read by one 128-bit load:
//   x  threshold (fp32 bits); a leaf with one (id, weight) entry keeps the weight here
//   y  feature id; a leaf keeps its class / target id (one entry) or the offset of its entries in the list
//   z  bits 0-2 mode (0 LEQ, 1 LT, 2 GTE, 3 GT, 4 EQ, 5 NEQ, 6 LEAF), bit 3 NaN-goes-true, bits 4.. the
//      number of (id, weight) entries of a leaf
//   w  true child (low 16 bits) and false child (high 16 bits), relative to the tree's first node
// Trees are contiguous; tree_off [T + 1] gives each tree's first node, tree_depth [T] the longest root-to-leaf
// path, and a walk makes at most that many steps, so a cyclic ensemble ends. Leaves with several entries
// point into a list of (id, weight bits) pairs. chunk_tree [C + 1] cuts the forest into runs of whole trees of
// at most kChunkNodes nodes; a tree larger than that is a chunk of its own and is walked in global memory.
//
// Row-parallel kernel: a block owns a tile of 256 / 128 / 64 rows, one per thread. The tile is staged once in
// LDS (16-byte global loads where X allows them) at an odd pitch, so lanes that read different features of
// their own rows spread over the banks; the tile shrinks until it fits, and past that X is read from global
// memory. The forest streams through a 16 KB LDS buffer chunk by chunk; each thread walks every tree of the
// chunk in tree order and adds the leaf entries into K <= 8 registers or into its own column of an LDS slab.
// The epilogue (average, base values, post-transform, argmax, label) runs on the accumulators.
//
// Tree-parallel kernel, for batches whose row tiles would leave most CUs idle: grid (row tiles, forest
// slices); a wave owns a row at a time, its lanes take the trees of the slice (lane, lane + 64, ...), read
// node records from global memory (the forest is L2-resident across blocks) and X broadcast from LDS. The
// lane partials are summed by an xor butterfly and written to a [slices, n, K] workspace; a second kernel
// sums the slices in order and runs the same epilogue. No atomics: results are bit-identical run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "nn_ops.h"

#define FW_HIP_CHECK(e)                                                                                \
  do {                                                                                                 \
    hipError_t _e = (e);                                                                               \
    if (_e != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e)); \
  } while (0)

namespace smlnn {
namespace {

constexpr int kThreads = 256;             // tree-parallel block; largest row tile
constexpr int kChunkNodes = kForestChunkNodes;
constexpr int kChunkBytes = kChunkNodes * 16;
constexpr int kTileBytes = 48 * 1024;     // X tile + accumulator slab
constexpr int kRegK = kForestRegK;        // up to here the scores of a row live in registers
constexpr int kMaxSlices = 64;
constexpr int kMaxRowsPerWave = 8;
constexpr int kLeaf = 6;

struct WalkArgs {
  const float* x;
  int64_t x_rs, n;
  const uint4* nodes;
  const uint2* list;
  const int32_t* tree_off;
  const int32_t* tree_depth;
  const int32_t* chunk_tree;
  int F, T, C, K;
  int pitch;                // LDS floats per staged row
  int vec;                  // X takes 16-byte loads
  int ts, rw;               // tree-parallel: trees per slice, rows per wave
  float* ws;
  int slices;
  // epilogue
  const float* base;
  float* out;
  int64_t* label;
  const int64_t* labels;
  int avg, post, binary, classifier;
};

// scores of one row: KR registers, or (KR = 0) every stride-th float from p
template <int KR>
struct Acc {
  float r[KR ? KR : 1];
  float* p;
  int stride;
  __device__ __forceinline__ void zero(int K) {
    if (KR) {
#pragma unroll
      for (int k = 0; k < KR; ++k) r[k] = 0.f;
    } else {
      for (int k = 0; k < K; ++k) p[static_cast<int64_t>(k) * stride] = 0.f;
    }
  }
  __device__ __forceinline__ void add(uint32_t id, float w) {
    if (KR == 1) {
      r[0] += w;
    } else if (KR) {
#pragma unroll
      for (int k = 0; k < KR; ++k)
        if (id == static_cast<uint32_t>(k)) r[k] += w;
    } else {
      p[static_cast<int64_t>(id) * stride] += w;
    }
  }
  __device__ __forceinline__ float& at(int k) { return KR ? r[k] : p[static_cast<int64_t>(k) * stride]; }
};

// the record a row ends on in one tree: at most depth steps from the root
template <class XF>
__device__ __forceinline__ uint4 walk(const uint4* __restrict__ tree, int depth, XF xf) {
  uint4 r = tree[0];
  for (int d = 0; d < depth && (r.z & 7u) != kLeaf; ++d) {
    const float v = xf(r.y), thr = __uint_as_float(r.x);
    const uint32_t mode = r.z & 7u;
    bool go = mode == 0 ? v <= thr : mode == 1 ? v < thr : mode == 2 ? v >= thr : mode == 3 ? v > thr
                                                                     : mode == 4 ? v == thr : v != thr;
    if (v != v) go = (r.z >> 3) & 1u;
    r = tree[go ? (r.w & 0xffffu) : (r.w >> 16)];
  }
  return r;
}

template <int KR>
__device__ __forceinline__ void leaf_add(const uint4& r, const uint2* __restrict__ list, Acc<KR>& acc) {
  if ((r.z & 7u) != kLeaf) return;  // a cyclic tree that never reached a leaf adds nothing
  const uint32_t cnt = r.z >> 4;
  if (cnt == 1) {
    acc.add(r.y, __uint_as_float(r.x));
  } else {
    for (uint32_t e = 0; e < cnt; ++e) {
      const uint2 it = list[r.y + e];
      acc.add(it.x, __uint_as_float(it.y));
    }
  }
}

__device__ __forceinline__ float sigmoidf(float s) { return 1.f / (1.f + expf(-s)); }

// fn(k) for k in [from, K): unrolled over the KR registers, or a plain loop over the slab
template <int KR, class Fn>
__device__ __forceinline__ void for_k(int K, int from, Fn fn) {
  if constexpr (KR != 0) {
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (k >= from && k < K) fn(k);
  } else {
    for (int k = from; k < K; ++k) fn(k);
  }
}

// average, base values, post-transform, argmax (lowest index on ties) and label of one row
template <int KR>
__device__ __forceinline__ void epilogue(const WalkArgs& a, int64_t row, Acc<KR>& acc) {
  const float t = static_cast<float>(a.T);
  for_k<KR>(a.K, 0, [&](int k) {
    float v = acc.at(k);
    if (a.avg) v = v / t;
    if (a.base) v += a.base[k];
    acc.at(k) = v;
  });
  if (a.binary) {
    const float s = acc.at(0);
    float lo = -s, hi = s;
    if (a.post == 1) {
      hi = sigmoidf(s);
      lo = 1.f - hi;
    }
    a.out[row * 2] = lo;
    a.out[row * 2 + 1] = hi;
    const int idx = s > 0.f ? 1 : 0;
    a.label[row] = a.labels ? a.labels[idx] : idx;
    return;
  }
  float best = acc.at(0);
  int idx = 0;
  for_k<KR>(a.K, 1, [&](int k) {
    const float v = acc.at(k);
    if (v > best || (v != v && best == best)) {
      best = v;
      idx = k;
    }
  });
  if (a.classifier) a.label[row] = a.labels ? a.labels[idx] : idx;
  float* o = a.out + row * a.K;
  if (a.post == 2) {
    float sum = 0.f;
    for_k<KR>(a.K, 0, [&](int k) {
      const float e = expf(acc.at(k) - best);
      acc.at(k) = e;
      sum += e;
    });
    for_k<KR>(a.K, 0, [&](int k) { o[k] = acc.at(k) / sum; });
  } else {
    for_k<KR>(a.K, 0, [&](int k) { o[k] = a.post == 1 ? sigmoidf(acc.at(k)) : acc.at(k); });
  }
}

// rows [row0, row0 + rows) of X into xt at a.pitch floats per row; rows past n are left alone
__device__ __forceinline__ void stage_x(const WalkArgs& a, int64_t row0, int rows, float* xt) {
  if (a.vec) {
    const int f4 = a.F / 4;
    for (int i = threadIdx.x; i < rows * f4; i += blockDim.x) {
      const int r = i / f4, c = (i - r * f4) * 4;
      if (row0 + r < a.n) {
        const float4 v = *reinterpret_cast<const float4*>(a.x + (row0 + r) * a.x_rs + c);
        float* d = xt + static_cast<int64_t>(r) * a.pitch + c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
    }
  } else {
    for (int i = threadIdx.x; i < rows * a.F; i += blockDim.x) {
      const int r = i / a.F, c = i - r * a.F;
      if (row0 + r < a.n) xt[static_cast<int64_t>(r) * a.pitch + c] = a.x[(row0 + r) * a.x_rs + c];
    }
  }
}

template <int KR, bool XL>
__global__ __launch_bounds__(kThreads) void forest_rows_kernel(const WalkArgs a) {
  extern __shared__ uint4 smem[];
  uint4* fl = smem;
  float* xt = reinterpret_cast<float*>(smem + kChunkNodes);
  const int R = blockDim.x, tid = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * R, row = row0 + tid;
  const bool active = row < a.n;
  if (XL) stage_x(a, row0, R, xt);
  Acc<KR> acc;
  acc.p = xt + (XL ? static_cast<int64_t>(R) * a.pitch : 0) + tid;
  acc.stride = R;
  acc.zero(a.K);
  const float* xrow = XL ? xt + static_cast<int64_t>(tid) * a.pitch : a.x + (active ? row : 0) * a.x_rs;
  auto xf = [&](uint32_t f) { return xrow[f]; };
  for (int c = 0; c < a.C; ++c) {
    const int t0 = a.chunk_tree[c], t1 = a.chunk_tree[c + 1];
    const int n0 = a.tree_off[t0], nn = a.tree_off[t1] - n0;
    if (nn <= kChunkNodes) {
      __syncthreads();  // the previous chunk's walks are done (and, first time round, the X tile is written)
      for (int i = tid; i < nn; i += R) fl[i] = a.nodes[n0 + i];
      __syncthreads();
      if (active)
        for (int t = t0; t < t1; ++t) leaf_add(walk(fl + (a.tree_off[t] - n0), a.tree_depth[t], xf), a.list, acc);
    } else {
      if (XL && c == 0) __syncthreads();
      if (active)
        for (int t = t0; t < t1; ++t) leaf_add(walk(a.nodes + a.tree_off[t], a.tree_depth[t], xf), a.list, acc);
    }
  }
  if (active) epilogue(a, row, acc);
}

template <int KR, bool XL>
__global__ __launch_bounds__(kThreads) void forest_trees_kernel(const WalkArgs a) {
  extern __shared__ uint4 smem[];
  float* xt = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int RT = 4 * a.rw;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * RT;
  if (XL) {
    stage_x(a, row0, RT, xt);
    __syncthreads();
  }
  Acc<KR> acc;
  acc.p = xt + (XL ? static_cast<int64_t>(RT) * a.pitch : 0) + tid;
  acc.stride = kThreads;
  const int slice = blockIdx.y, t0 = slice * a.ts, t1 = min(a.T, t0 + a.ts);
  for (int j = 0; j < a.rw; ++j) {
    const int r = wave * a.rw + j;
    const int64_t row = row0 + r;
    if (row >= a.n) break;  // the same for every lane of the wave
    const float* xrow = XL ? xt + static_cast<int64_t>(r) * a.pitch : a.x + row * a.x_rs;
    auto xf = [&](uint32_t f) { return xrow[f]; };
    acc.zero(a.K);
    for (int t = t0 + lane; t < t1; t += 64)
      leaf_add(walk(a.nodes + a.tree_off[t], a.tree_depth[t], xf), a.list, acc);
    float* w = a.ws + (static_cast<int64_t>(slice) * a.n + row) * a.K;
    for_k<KR>(a.K, 0, [&](int k) {
      float v = acc.at(k);
#pragma unroll
      for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
      if (lane == 0) w[k] = v;
    });
  }
}

// sums the slices of the workspace in order into slice 0 and runs the epilogue there
__global__ __launch_bounds__(kThreads) void forest_finish_kernel(const WalkArgs a) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (row >= a.n) return;
  Acc<0> acc;
  acc.p = a.ws + row * a.K;
  acc.stride = 1;
  for (int k = 0; k < a.K; ++k) {
    float s = acc.at(k);
    for (int sl = 1; sl < a.slices; ++sl) s += a.ws[(static_cast<int64_t>(sl) * a.n + row) * a.K + k];
    acc.at(k) = s;
  }
  epilogue(a, row, acc);
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

struct Plan {
  int shape = 0;  // 1 row-parallel, 2 tree-parallel
  int tile = 0;   // row-parallel: rows per block
  bool x_lds = false;
  int slices = 1, ts = 0, rw = 1;
  size_t lds = 0;
};

int64_t slab_floats(int K) { return K > kRegK ? K : 0; }

bool plan_rows(int F, int K, Plan* p) {
  const int64_t pitch = static_cast<int64_t>(F) | 1, slab = slab_floats(K);
  for (int pass = 0; pass < 2; ++pass)  // with the X tile, then without
    for (int R = 256; R >= 64; R /= 2) {
      const int64_t bytes = R * ((pass == 0 ? pitch : 0) + slab) * 4;
      if (bytes <= kTileBytes) {
        p->shape = 1; p->tile = R; p->x_lds = pass == 0; p->lds = kChunkBytes + static_cast<size_t>(bytes);
        return true;
      }
    }
  return false;
}

bool plan_trees(int64_t n, int F, int T, int K, int cus, Plan* p) {
  const int64_t slab = slab_floats(K) * kThreads * 4;
  if (slab > kTileBytes) return false;
  const int want = std::min((T + 63) / 64, kMaxSlices);
  p->ts = (T + want - 1) / want;
  p->slices = (T + p->ts - 1) / p->ts;
  const int64_t rw = (n * p->slices + 8LL * cus - 1) / (8LL * cus);
  p->rw = static_cast<int>(std::min<int64_t>(std::max<int64_t>(rw, 1), kMaxRowsPerWave));
  const int64_t xb = 4LL * p->rw * F * 4;
  p->x_lds = xb + slab <= kTileBytes;
  p->lds = static_cast<size_t>((p->x_lds ? xb : 0) + slab);
  p->shape = 2;
  return true;
}

// launch: 0 by batch size, 1 row-parallel, 2 tree-parallel
bool make_plan(int64_t n, int F, int T, int K, int launch, Plan* p) {
  if (n <= 0 || F <= 0 || T <= 0 || K <= 0 || launch < 0 || launch > 2) return false;
  const int cus = cu_count();
  Plan rows, trees;
  const bool rows_ok = plan_rows(F, K, &rows), trees_ok = plan_trees(n, F, T, K, cus, &trees);
  const bool fills = rows_ok && (n + rows.tile - 1) / rows.tile >= static_cast<int64_t>(kForestRowBlocksPerCu) * cus;
  if (launch == 1 || (launch == 0 && rows_ok && (!trees_ok || fills))) {
    if (!rows_ok || (n + rows.tile - 1) / rows.tile > INT32_MAX) return false;
    *p = rows;
    return true;
  }
  if (!trees_ok || (n + 4 * trees.rw - 1) / (4 * trees.rw) > INT32_MAX) return false;
  *p = trees;
  return true;
}

template <int KR>
void launch_kr(const WalkArgs& a, const Plan& p, hipStream_t s) {
  if (p.shape == 1) {
    const dim3 grid(static_cast<unsigned>((a.n + p.tile - 1) / p.tile));
    if (p.x_lds) hipLaunchKernelGGL((forest_rows_kernel<KR, true>), grid, dim3(p.tile), p.lds, s, a);
    else hipLaunchKernelGGL((forest_rows_kernel<KR, false>), grid, dim3(p.tile), p.lds, s, a);
    return;
  }
  const dim3 grid(static_cast<unsigned>((a.n + 4 * p.rw - 1) / (4 * p.rw)), p.slices);
  if (p.x_lds) hipLaunchKernelGGL((forest_trees_kernel<KR, true>), grid, dim3(kThreads), p.lds, s, a);
  else hipLaunchKernelGGL((forest_trees_kernel<KR, false>), grid, dim3(kThreads), p.lds, s, a);
  hipLaunchKernelGGL(forest_finish_kernel, dim3(static_cast<unsigned>((a.n + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, a);
}

}  // namespace

int ForestWalkPlan(int64_t n, int F, int T, int K, int launch, int* slices) {
  Plan p;
  if (!make_plan(n, F, T, K, launch, &p)) return -4;
  *slices = p.shape == 2 ? p.slices : 0;
  return p.shape;
}

int ForestWalk(const ForestArgs& f, void* stream) {
  if (!f.x || !f.nodes || !f.tree_off || !f.tree_depth || !f.chunk_tree || !f.out || f.x_rs < 0 || f.C <= 0) return -4;
  if (f.post < 0 || f.post > 2 || (f.binary && (f.K != 1 || !f.classifier)) || (f.classifier && !f.label)) return -4;
  Plan p;
  if (!make_plan(f.n, f.F, f.T, f.K, f.launch, &p)) return -4;
  if (p.shape == 2 && (!f.ws || f.ws_floats < static_cast<int64_t>(p.slices) * f.n * f.K)) return -4;
  WalkArgs a;
  a.x = f.x; a.x_rs = f.x_rs; a.n = f.n;
  a.nodes = static_cast<const uint4*>(f.nodes); a.list = static_cast<const uint2*>(f.list);
  a.tree_off = f.tree_off; a.tree_depth = f.tree_depth; a.chunk_tree = f.chunk_tree;
  a.F = f.F; a.T = f.T; a.C = f.C; a.K = f.K;
  a.pitch = p.shape == 1 ? (f.F | 1) : f.F;
  a.vec = f.F % 4 == 0 && f.x_rs % 4 == 0 && reinterpret_cast<uintptr_t>(f.x) % 16 == 0;
  a.ts = p.ts; a.rw = p.rw; a.ws = f.ws; a.slices = p.slices;
  a.base = f.base; a.out = f.out; a.label = f.label; a.labels = f.labels;
  a.avg = f.average; a.post = f.post; a.binary = f.binary; a.classifier = f.classifier;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (f.K == 1) launch_kr<1>(a, p, s);
  else if (f.K <= kRegK) launch_kr<kRegK>(a, p, s);
  else launch_kr<0>(a, p, s);
  FW_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace smlnn
