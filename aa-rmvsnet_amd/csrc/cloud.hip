// Point-cloud evaluation for gfx950 (include/aarmvs.h, "Point-cloud evaluation"): the grid keys of
// a cloud, the truncated exact nearest neighbour of every query point in a key-sorted target cloud,
// the fixed-order statistics of the distances, the per-voxel centroids of a key-sorted cloud, and
// the DTU protocol's greedy thinning (in parallel rounds) and region flags.
// All arithmetic is float64 with every operation rounded on its own (built with -ffp-contract=off;
// the __d*_rn forms say so where the definition names an order).  No atomics anywhere: every
// result is the same on every run.
//
// The query kernel is one thread per query (the caller sorts the queries by the same key, so the
// threads of a wave walk the same target spans and their loads hit the same cache lines).  Per
// ring and per (i_y, i_z) row: one binary search in target_keys for the row's first cell, then a
// linear scan that reads key and point until the key leaves the row's x-span.
// Algorithmic bytes per query: 12 read + 4 or 8 written, and per visited row about log2(m) keys
// (8 B each, the upper levels shared by the whole wave) + 20 (+ 4 with ids) per scanned target.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "aarmvs_internal.h"

namespace aarmvs {

namespace {

constexpr int kCloudThreads = 256;
constexpr long long kNoKey = 0x7fffffffffffffffLL;   // INT64_MAX: not in the grid
constexpr double kAxisCells = 2097152.0;             // 2^21

__device__ __forceinline__ double cell_quotient(double p, double o, double cell) {
  return floor(__ddiv_rn(__dsub_rn(p, o), cell));
}

// the cell index of coordinate p, or false when it is not in [0, 2^21) (NaN and +-inf included)
__device__ __forceinline__ bool cell_of(double p, double o, double cell, int& i) {
  const double t = cell_quotient(p, o, cell);
  if (!(t >= 0.0 && t < kAxisCells)) return false;
  i = (int)t;
  return true;
}

struct Grid {
  double o[3];
  double cell;
};

__global__ void __launch_bounds__(kCloudThreads)
cloud_keys_kernel(const float* __restrict__ xyz, long long n, Grid g, long long* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
  if (i >= n) return;
  const float* p = xyz + (size_t)i * 3;
  int c[3] = {0, 0, 0};
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) in = cell_of((double)p[a], g.o[a], g.cell, c[a]) && in;
  keys[i] = in ? ((long long)c[2] << 42) | ((long long)c[1] << 21) | (long long)c[0] : kNoKey;
}

struct NnArgs {
  const float* query;
  const float* target;
  const long long* keys;
  const int* ids;
  long long nq, m;
  Grid g;
  double reach;        // max_dist (1 + 2^-40): what the per-axis cell bounds are taken at
  double cell_shrunk;  // cell (1 - 2^-20): the stopping test's ring width
  double max_d2;       // (double) max_dist * (double) max_dist
  float* dist;
  int* index;
};

// first j in [0, m) with keys[j] >= key (m if none)
__device__ __forceinline__ long long lower_bound(const long long* __restrict__ keys, long long m,
                                                 long long key) {
  long long lo = 0, hi = m;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kCloudThreads) cloud_nn_kernel(NnArgs a) {
  const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
  if (i >= a.nq) return;
  const float* qp = a.query + (size_t)i * 3;
  const double q[3] = {(double)qp[0], (double)qp[1], (double)qp[2]};
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  float out_d = __int_as_float(0x7f800000);
  int out_i = -1;
  int c[3] = {0, 0, 0}, lo[3], hi[3];
  bool finite = true, in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    finite = finite && fabs(q[k]) < inf;
    in = cell_of(q[k], a.g.o[k], a.g.cell, c[k]) && in;
  }
  if (!finite) out_d = __int_as_float(0x7fc00000);
  if (finite && in) {
    // Per axis, the cells that can hold a point within max_dist: the cell function is monotone in
    // the coordinate, so every such target lies in [cell(q - reach), cell(q + reach)].
    int rings = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double tl = cell_quotient(__dsub_rn(q[k], a.reach), a.g.o[k], a.g.cell);
      const double th = cell_quotient(__dadd_rn(q[k], a.reach), a.g.o[k], a.g.cell);
      lo[k] = (int)fmin(fmax(tl, 0.0), (double)c[k]);
      hi[k] = (int)fmax(fmin(th, kAxisCells - 1.0), (double)c[k]);
      rings = max(rings, max(c[k] - lo[k], hi[k] - c[k]));
    }
    double best = inf;
    int best_id = 0x7fffffff;
    // the targets of row (iy, iz) with x-cell in [xa, xb]
    auto scan = [&](int iy, int iz, int xa, int xb) {
      const long long base = ((long long)iz << 42) | ((long long)iy << 21);
      const long long last = base | (long long)xb;
      for (long long j = lower_bound(a.keys, a.m, base | (long long)xa); j < a.m && a.keys[j] <= last; ++j) {
        const float* t = a.target + (size_t)j * 3;
        const double dx = q[0] - (double)t[0], dy = q[1] - (double)t[1], dz = q[2] - (double)t[2];
        const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        const int id = a.ids ? a.ids[j] : (int)j;
        if (d2 < best || (d2 == best && id < best_id)) {
          best = d2;
          best_id = id;
        }
      }
    };
    for (int k = 0; k <= rings; ++k) {
      for (int dz = -k; dz <= k; ++dz) {
        const int iz = c[2] + dz;
        if (iz < lo[2] || iz > hi[2]) continue;
        for (int dy = -k; dy <= k; ++dy) {
          const int iy = c[1] + dy;
          if (iy < lo[1] || iy > hi[1]) continue;
          if (abs(dz) == k || abs(dy) == k) {   // a row of the shell: its whole x-span
            scan(iy, iz, max(c[0] - k, lo[0]), min(c[0] + k, hi[0]));
          } else {                              // an inner row: the shell's two end cells
            if (c[0] - k >= lo[0]) scan(iy, iz, c[0] - k, c[0] - k);
            if (c[0] + k <= hi[0]) scan(iy, iz, c[0] + k, c[0] + k);
          }
        }
      }
      // Every target not looked at yet is k + 1 or more cells away along some axis, so its
      // distance is above k * cell_shrunk (the 2^-20 covers the quotients' and d2's roundings,
      // below 2^-30 together) and its d2 strictly above the bound: no tie is lost.  Not at k = 0,
      // where the bound is 0 and an equal, lower-id target may sit in a neighbouring cell.
      if (k >= 1) {
        const double w = __dmul_rn((double)k, a.cell_shrunk);
        if (best <= __dmul_rn(w, w)) break;
      }
    }
    if (best <= a.max_d2) {
      out_d = (float)sqrt(best);
      out_i = best_id;
    }
  }
  a.dist[i] = out_d;
  if (a.index) a.index[i] = out_i;
}

// ---------------------------------------------------------------------------------
// Statistics of a distance array: a block owns kStatChunk consecutive values, a thread adds its
// kStatChunk / 256 values in index order, the block sums in a fixed order (xor butterfly per
// wave, the waves in index order), and one block adds the per-block partials the same way.
// ---------------------------------------------------------------------------------
constexpr int kStatRounds = 16, kStatChunk = kCloudThreads * kStatRounds;
constexpr int kStatVals = 3 + AARMVS_MAX_THRESHOLDS;

struct CloudThresholds {
  float v[AARMVS_MAX_THRESHOLDS];
};

__device__ inline void stat_block_sum(double (&v)[kStatVals], double* lds) {
#pragma unroll
  for (int k = 0; k < kStatVals; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kStatVals; ++k) lds[wave * kStatVals + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kStatVals; ++k) {
      double s = lds[k];
      for (int w = 1; w < kCloudThreads / 64; ++w) s += lds[w * kStatVals + k];
      v[k] = s;
    }
  }
}

__global__ void __launch_bounds__(kCloudThreads)
cloud_stats_kernel(const float* __restrict__ dist, long long n, CloudThresholds thr, int nthr,
                   double* __restrict__ part) {
  __shared__ double lds[(kCloudThreads / 64) * kStatVals];
  double acc[kStatVals];
#pragma unroll
  for (int k = 0; k < kStatVals; ++k) acc[k] = 0.0;
  const long long base = (long long)blockIdx.x * kStatChunk + threadIdx.x;
  for (int r = 0; r < kStatRounds; ++r) {
    const long long i = base + (long long)r * kCloudThreads;
    if (i >= n) break;
    const float d = dist[i];
    if (d != d) {
      acc[2] += 1.0;
    } else if (fabsf(d) < __int_as_float(0x7f800000)) {
      acc[0] += 1.0;
      acc[1] += (double)d;
#pragma unroll
      for (int k = 0; k < AARMVS_MAX_THRESHOLDS; ++k)
        if (k < nthr && d < thr.v[k]) acc[3 + k] += 1.0;
    }
  }
  stat_block_sum(acc, lds);
  if (threadIdx.x == 0) {
    double* o = part + (size_t)blockIdx.x * kStatVals;
#pragma unroll
    for (int k = 0; k < kStatVals; ++k) o[k] = acc[k];
  }
}

__global__ void __launch_bounds__(kCloudThreads)
cloud_stats_reduce_kernel(const double* __restrict__ part, int nblk, int nthr, double* __restrict__ out) {
  __shared__ double lds[(kCloudThreads / 64) * kStatVals];
  double acc[kStatVals];
#pragma unroll
  for (int k = 0; k < kStatVals; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < nblk; i += kCloudThreads) {
    const double* o = part + (size_t)i * kStatVals;
#pragma unroll
    for (int k = 0; k < kStatVals; ++k) acc[k] += o[k];
  }
  stat_block_sum(acc, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kStatVals; ++k)
      if (k < 3 + nthr) out[k] = acc[k];
  }
}

// ---------------------------------------------------------------------------------
// Voxel centroids of a key-sorted cloud, by the count / exclusive scan / rank scheme of
// aarmvs_fusion_points: point i STARTS a cell when its key is not INT64_MAX and differs from
// point i - 1's.  A block owns kVoxChunk consecutive points in kVoxRounds rounds of one point per
// thread; the thread of a starting point adds the cell's points in sorted order (they are
// consecutive) and writes the centroid at the start's rank.
// ---------------------------------------------------------------------------------
constexpr int kVoxRounds = 4, kVoxWaves = kCloudThreads / 64, kVoxChunk = kCloudThreads * kVoxRounds;

__device__ __forceinline__ bool cell_start(const long long* __restrict__ keys, long long n, long long i) {
  if (i >= n) return false;
  const long long k = keys[i];
  return k != kNoKey && (i == 0 || keys[i - 1] != k);
}

__global__ void __launch_bounds__(kCloudThreads)
voxel_count_kernel(const long long* __restrict__ keys, long long n, int* __restrict__ block_cnt) {
  __shared__ int wcnt[kVoxWaves];
  const long long base = (long long)blockIdx.x * kVoxChunk;
  int c = 0;
#pragma unroll
  for (int r = 0; r < kVoxRounds; ++r)
    c += __popcll(__ballot(cell_start(keys, n, base + r * kCloudThreads + threadIdx.x)));
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kVoxWaves; ++w) t += wcnt[w];
    block_cnt[blockIdx.x] = t;
  }
}

// cnt[0 .. n) -> its exclusive prefix sums, in place; *total = the sum (< 2^31: the points are)
__global__ void __launch_bounds__(kCloudThreads) voxel_scan_kernel(int* __restrict__ cnt, int n,
                                                                   long long* __restrict__ total) {
  __shared__ int wsum[kCloudThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += kCloudThreads) {
    const int i = base + threadIdx.x;
    const int v = i < n ? cnt[i] : 0;
    int s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(s, d);
      if (lane >= d) s += t;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    int before = 0, tile = 0;
#pragma unroll
    for (int w = 0; w < kCloudThreads / 64; ++w) {
      before += w < wave ? wsum[w] : 0;
      tile += wsum[w];
    }
    if (i < n) cnt[i] = carry + before + s - v;
    carry += tile;
    __syncthreads();   // wsum is rewritten by the next tile
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ void __launch_bounds__(kCloudThreads)
voxel_write_kernel(const float* __restrict__ xyz, const long long* __restrict__ keys, long long n,
                   const int* __restrict__ block_off, float* __restrict__ out, long long capacity) {
  __shared__ int wcnt[kVoxRounds][kVoxWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * kVoxChunk;
  bool start[kVoxRounds];
  int below[kVoxRounds];
#pragma unroll
  for (int r = 0; r < kVoxRounds; ++r) {
    start[r] = cell_start(keys, n, base + r * kCloudThreads + threadIdx.x);
    const unsigned long long b = __ballot(start[r]);
    below[r] = __popcll(b & ((1ULL << lane) - 1ULL));
    if (lane == 0) wcnt[r][wave] = __popcll(b);
  }
  __syncthreads();
  long long acc = block_off[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kVoxRounds; ++r) {
    int before = 0, round = 0;
#pragma unroll
    for (int w = 0; w < kVoxWaves; ++w) {
      before += w < wave ? wcnt[r][w] : 0;
      round += wcnt[r][w];
    }
    const long long rank = acc + before + below[r];
    acc += round;
    if (!start[r] || rank >= capacity) continue;
    const long long i0 = base + r * kCloudThreads + threadIdx.x;
    const long long key = keys[i0];
    double s[3] = {0.0, 0.0, 0.0};
    long long j = i0;
    do {
      const float* p = xyz + (size_t)j * 3;
      s[0] += (double)p[0];
      s[1] += (double)p[1];
      s[2] += (double)p[2];
      ++j;
    } while (j < n && keys[j] == key);
    const double cnt = (double)(j - i0);
    float* o = out + (size_t)rank * 3;
    o[0] = (float)__ddiv_rn(s[0], cnt);
    o[1] = (float)__ddiv_rn(s[1], cnt);
    o[2] = (float)__ddiv_rn(s[2], cnt);
  }
}

// ---------------------------------------------------------------------------------
// Greedy thinning in parallel rounds (include/aarmvs.h, "DTU protocol"): one thread per point of
// the key-sorted cloud.  A decided point copies its state byte through and is done, which is what
// carries the later rounds (a byte read and a byte written per point).  An undecided point walks
// the rows of its box as cloud_nn_kernel does and tests per candidate the cheap things first: the
// rank (4 B), the state byte, then d2 (12 B).  A round reads st_in only and writes st_out only.
// Per block, as plain stores: the number of its points still undecided after the round, and the
// last round of this call at whose start the block held an undecided point.
// ---------------------------------------------------------------------------------
constexpr unsigned char kUndecided = 0, kKept = 1, kRemoved = 2;
constexpr long long kAxisMask = (1LL << AARMVS_CLOUD_AXIS_BITS) - 1;

__global__ void __launch_bounds__(kCloudThreads)
thin_init_kernel(const long long* __restrict__ keys, long long n, unsigned char* __restrict__ st) {
  const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
  if (i < n) st[i] = keys[i] == kNoKey ? kRemoved : kUndecided;
}

struct ThinArgs {
  const float* xyz;
  const long long* keys;
  const int* rank;
  long long n;
  Grid g;
  double reach;   // r (1 + 2^-40)
  double r2;      // (double) r * (double) r
  const unsigned char* st_in;
  unsigned char* st_out;
  int* block_cnt;
  int* block_last;
  int round;      // 1-based within the call
};

// the new state of undecided point i (in the grid: its key holds its cell)
__device__ __forceinline__ unsigned char thin_decide(const ThinArgs& a, long long i) {
  const float* pp = a.xyz + (size_t)i * 3;
  const double p[3] = {(double)pp[0], (double)pp[1], (double)pp[2]};
  const long long key = a.keys[i];
  const int c[3] = {(int)(key & kAxisMask), (int)((key >> 21) & kAxisMask), (int)(key >> 42)};
  const int my = a.rank[i];
  int lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double tl = cell_quotient(__dsub_rn(p[k], a.reach), a.g.o[k], a.g.cell);
    const double th = cell_quotient(__dadd_rn(p[k], a.reach), a.g.o[k], a.g.cell);
    lo[k] = (int)fmin(fmax(tl, 0.0), (double)c[k]);
    hi[k] = (int)fmax(fmin(th, kAxisCells - 1.0), (double)c[k]);
  }
  bool waits = false;   // an undecided lower-ranked neighbour was seen
  for (int iz = lo[2]; iz <= hi[2]; ++iz) {
    for (int iy = lo[1]; iy <= hi[1]; ++iy) {
      const long long base = ((long long)iz << 42) | ((long long)iy << 21);
      const long long last = base | (long long)hi[0];
      for (long long j = lower_bound(a.keys, a.n, base | (long long)lo[0]); j < a.n && a.keys[j] <= last; ++j) {
        if (a.rank[j] >= my) continue;   // (the point itself included)
        const unsigned char s = a.st_in[j];
        if (s == kRemoved || (s == kUndecided && waits)) continue;
        const float* t = a.xyz + (size_t)j * 3;
        const double dx = p[0] - (double)t[0], dy = p[1] - (double)t[1], dz = p[2] - (double)t[2];
        const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
        if (!(d2 <= a.r2)) continue;
        if (s == kKept) return kRemoved;
        waits = true;
      }
    }
  }
  return waits ? kUndecided : kKept;
}

__global__ void __launch_bounds__(kCloudThreads) thin_round_kernel(ThinArgs a) {
  const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
  unsigned char before = kRemoved, after = kRemoved;
  if (i < a.n) {
    before = after = a.st_in[i];
    if (before == kUndecided) after = thin_decide(a, i);
    a.st_out[i] = after;
  }
  const int active = __syncthreads_or(before == kUndecided);
  const int left = __syncthreads_count(after == kUndecided);
  if (threadIdx.x == 0) {
    a.block_cnt[blockIdx.x] = left;
    if (a.round == 1 || active) a.block_last[blockIdx.x] = active ? a.round : 0;
  }
}

// out[0] = the sum of block_cnt, out[1] = the maximum of block_last, over nblk blocks (integers: any
// order gives the same bits; the order is fixed all the same)
__global__ void __launch_bounds__(kCloudThreads)
thin_reduce_kernel(const int* __restrict__ block_cnt, const int* __restrict__ block_last, int nblk,
                   long long* __restrict__ out) {
  __shared__ long long wsum[kCloudThreads / 64];
  __shared__ int wmax[kCloudThreads / 64];
  long long s = 0;
  int m = 0;
  for (int i = threadIdx.x; i < nblk; i += kCloudThreads) {
    s += block_cnt[i];
    m = max(m, block_last[i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    m = max(m, __shfl_xor(m, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = s;
    wmax[threadIdx.x >> 6] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kCloudThreads / 64; ++w) {
      s += wsum[w];
      m = max(m, wmax[w]);
    }
    out[0] = s;
    out[1] = m;
  }
}

// ---------------------------------------------------------------------------------
// Region flags of a cloud (include/aarmvs.h, "Region tests"): one thread per point.
// ---------------------------------------------------------------------------------
struct RegionArgs {
  double lo[3], hi[3];   // BB[0] - patch, BB[1] + 2 patch
  double bb0[3];
  double res;
  double plane[4];
  int dims[3];
  int has_box, has_plane;
  const unsigned char* mask;
};

__global__ void __launch_bounds__(kCloudThreads)
cloud_regions_kernel(const float* __restrict__ xyz, long long n, RegionArgs a, unsigned char* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * kCloudThreads + threadIdx.x;
  if (i >= n) return;
  const float* pp = xyz + (size_t)i * 3;
  const double p[3] = {(double)pp[0], (double)pp[1], (double)pp[2]};
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  unsigned char f = 0;
  if (fabs(p[0]) < inf && fabs(p[1]) < inf && fabs(p[2]) < inf) {
    if (a.has_box) {
      bool in_box = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) in_box = in_box && p[k] >= a.lo[k] && p[k] < a.hi[k];
      if (in_box) {
        f |= 1;
        if (a.mask) {
          long long g[3];
          bool in = true;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double t = rint(__ddiv_rn(__dsub_rn(p[k], a.bb0[k]), a.res));
            in = in && t >= 0.0 && t < (double)a.dims[k];
            g[k] = in ? (long long)t : 0;
          }
          if (in && a.mask[(g[0] * a.dims[1] + g[1]) * a.dims[2] + g[2]] != 0) f |= 2;
        }
      }
    }
    if (a.has_plane) {
      const double s = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a.plane[0], p[0]), __dmul_rn(a.plane[1], p[1])),
                                           __dmul_rn(a.plane[2], p[2])), a.plane[3]);
      if (s > 0.0) f |= 4;
    }
  }
  flags[i] = f;
}

int blocks_of(long long n, int chunk) { return (int)((n + chunk - 1) / chunk); }

Grid make_grid(const double* origin, double cell) {
  Grid g;
  for (int a = 0; a < 3; ++a) g.o[a] = origin[a];
  g.cell = cell;
  return g;
}

}  // namespace

// (all of these are timed under the points' profile id: the list of kernel names is fixed)
static hipError_t launch_cloud_keys(const float* xyz, long long n, const double* origin, double cell,
                                    long long* keys, hipStream_t s) {
  if (n == 0) return hipSuccess;
  ProfScope ps(s, K_FUSION_POINTS);
  hipLaunchKernelGGL(cloud_keys_kernel, dim3(blocks_of(n, kCloudThreads)), dim3(kCloudThreads), 0, s, xyz, n,
                     make_grid(origin, cell), keys);
  return hipGetLastError();
}

static hipError_t launch_cloud_nn(const aarmvs_cloud_nn_args* in, hipStream_t s) {
  if (in->nq == 0) return hipSuccess;
  NnArgs a{};
  a.query = in->query;
  a.target = in->target;
  a.keys = in->target_keys;
  a.ids = in->target_ids;
  a.nq = in->nq;
  a.m = in->m;
  a.g = make_grid(in->origin, in->cell);
  const double md = (double)in->max_dist;
  a.reach = md * (1.0 + 0x1p-40);
  a.cell_shrunk = in->cell * (1.0 - 0x1p-20);
  a.max_d2 = md * md;
  a.dist = in->dist_out;
  a.index = in->index_out;
  ProfScope ps(s, K_FUSION_POINTS);
  hipLaunchKernelGGL(cloud_nn_kernel, dim3(blocks_of(a.nq, kCloudThreads)), dim3(kCloudThreads), 0, s, a);
  return hipGetLastError();
}

static size_t cloud_stats_scratch_bytes(long long n) {
  return ((size_t)std::max(1, blocks_of(n, kStatChunk)) * kStatVals * sizeof(double) + 255) / 256 * 256;
}

static hipError_t launch_cloud_stats(const float* dist, long long n, const float* thresholds, int nthr, double* out,
                                     void* scratch, hipStream_t s) {
  const int nblk = blocks_of(n, kStatChunk);
  double* part = static_cast<double*>(scratch);
  CloudThresholds thr{};
  for (int k = 0; k < nthr; ++k) thr.v[k] = thresholds[k];
  ProfScope ps(s, K_FUSION_POINTS);
  if (nblk > 0) {
    hipLaunchKernelGGL(cloud_stats_kernel, dim3(nblk), dim3(kCloudThreads), 0, s, dist, n, thr, nthr, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(cloud_stats_reduce_kernel, dim3(1), dim3(kCloudThreads), 0, s, part, nblk, nthr, out);
  return hipGetLastError();
}

static size_t cloud_voxel_workspace_bytes(long long n) {
  return ((size_t)std::max(1, blocks_of(n, kVoxChunk)) * sizeof(int) + 255) / 256 * 256;
}

static hipError_t launch_cloud_voxel_centroids(const float* xyz, const long long* keys, long long n, float* out,
                                               long long capacity, long long* count, void* workspace,
                                               hipStream_t s) {
  int* blk = static_cast<int*>(workspace);
  const int nb = blocks_of(n, kVoxChunk);
  ProfScope ps(s, K_FUSION_POINTS);
  hipError_t e = hipSuccess;
  if (nb > 0) {
    hipLaunchKernelGGL(voxel_count_kernel, dim3(nb), dim3(kCloudThreads), 0, s, keys, n, blk);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(kCloudThreads), 0, s, blk, nb, count);
  if ((e = hipGetLastError()) != hipSuccess || nb == 0) return e;
  hipLaunchKernelGGL(voxel_write_kernel, dim3(nb), dim3(kCloudThreads), 0, s, xyz, keys, n, blk, out,
                     capacity);
  return hipGetLastError();
}

// two ints per block of kCloudThreads points: the undecided count and the last active round
static size_t cloud_thin_scratch_bytes(long long n) {
  return ((size_t)std::max(1, blocks_of(n, kCloudThreads)) * 2 * sizeof(int) + 255) / 256 * 256;
}

static hipError_t launch_cloud_thin(const aarmvs_cloud_thin_args* in, int rounds, hipStream_t s) {
  const int nb = blocks_of(in->n, kCloudThreads);
  int* block_cnt = static_cast<int*>(in->scratch);
  int* block_last = block_cnt + std::max(1, nb);
  ProfScope ps(s, K_FUSION_POINTS);
  hipError_t e = hipSuccess;
  if (nb > 0) {
    if (in->init) {
      hipLaunchKernelGGL(thin_init_kernel, dim3(nb), dim3(kCloudThreads), 0, s, in->keys, in->n,
                         in->state[in->which]);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    ThinArgs a{};
    a.xyz = in->xyz;
    a.keys = in->keys;
    a.rank = in->rank;
    a.n = in->n;
    a.g = make_grid(in->origin, in->cell);
    const double r = (double)in->r;
    a.reach = r * (1.0 + 0x1p-40);
    a.r2 = r * r;
    a.block_cnt = block_cnt;
    a.block_last = block_last;
    for (int k = 1; k <= rounds; ++k) {
      a.st_in = in->state[(in->which + k - 1) & 1];
      a.st_out = in->state[(in->which + k) & 1];
      a.round = k;
      hipLaunchKernelGGL(thin_round_kernel, dim3(nb), dim3(kCloudThreads), 0, s, a);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  hipLaunchKernelGGL(thin_reduce_kernel, dim3(1), dim3(kCloudThreads), 0, s, block_cnt, block_last, nb,
                     in->remaining);
  return hipGetLastError();
}

static hipError_t launch_cloud_regions(const float* xyz, long long n, const unsigned char* mask, const int* dims,
                                       const double* bb, double res, double patch, const double* plane,
                                       unsigned char* flags, hipStream_t s) {
  if (n == 0) return hipSuccess;
  RegionArgs a{};
  a.has_box = bb != nullptr;
  a.has_plane = plane != nullptr;
  a.mask = mask;
  a.res = mask ? res : 1.0;
  for (int k = 0; k < 3; ++k) {
    if (bb) {
      a.bb0[k] = bb[k];
      a.lo[k] = bb[k] - patch;
      a.hi[k] = bb[3 + k] + 2.0 * patch;
    }
    a.dims[k] = mask ? dims[k] : 1;
  }
  for (int k = 0; k < 4; ++k) a.plane[k] = plane ? plane[k] : 0.0;
  ProfScope ps(s, K_FUSION_POINTS);
  hipLaunchKernelGGL(cloud_regions_kernel, dim3(blocks_of(n, kCloudThreads)), dim3(kCloudThreads), 0, s, xyz, n, a,
                     flags);
  return hipGetLastError();
}

}  // namespace aarmvs

using namespace aarmvs;

extern "C" {

static bool cloud_count_ok(long long n) { return n >= 0 && n < (1LL << 31); }
static bool cloud_cell_ok(double cell) { return std::isfinite(cell) && cell > 0.0; }
static bool cloud_origin_ok(const double* o) {
  return std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]);
}

int aarmvs_cloud_keys(const float* xyz, long long n, const double* origin, double cell, long long* keys_out,
                      hipStream_t stream) {
  if (!cloud_count_ok(n)) return fail(AARMVS_ERR_INVALID, "cloud_keys: need 0 <= n < 2^31");
  if (!origin || (n > 0 && (!xyz || !keys_out)))
    return fail(AARMVS_ERR_INVALID, "cloud_keys: null pointer argument");
  if (!cloud_origin_ok(origin)) return fail(AARMVS_ERR_INVALID, "cloud_keys: origin must be finite");
  if (!cloud_cell_ok(cell)) return fail(AARMVS_ERR_INVALID, "cloud_keys: cell must be finite and > 0");
  if (n > 0 && ranges_overlap(keys_out, 8 * (size_t)n, xyz, 12 * (size_t)n))
    return fail(AARMVS_ERR_INVALID, "cloud_keys: keys_out must not alias xyz");
  return launched(launch_cloud_keys(xyz, n, origin, cell, keys_out, stream), "cloud_keys");
}

int aarmvs_cloud_nn(const aarmvs_cloud_nn_args* a, hipStream_t stream) {
  if (!a) return fail(AARMVS_ERR_INVALID, "cloud_nn: null args");
  if (!cloud_count_ok(a->nq) || !cloud_count_ok(a->m))
    return fail(AARMVS_ERR_INVALID, "cloud_nn: need 0 <= nq, m < 2^31");
  if ((a->nq > 0 && (!a->query || !a->dist_out)) || (a->m > 0 && (!a->target || !a->target_keys)))
    return fail(AARMVS_ERR_INVALID, "cloud_nn: null pointer argument");
  if (!cloud_origin_ok(a->origin)) return fail(AARMVS_ERR_INVALID, "cloud_nn: origin must be finite");
  if (!cloud_cell_ok(a->cell)) return fail(AARMVS_ERR_INVALID, "cloud_nn: cell must be finite and > 0");
  if (!(a->max_dist >= 0.0f) || std::isinf(a->max_dist))
    return fail(AARMVS_ERR_INVALID, "cloud_nn: max_dist must be finite and >= 0");
  if ((double)a->max_dist / a->cell > (double)AARMVS_CLOUD_MAX_RINGS)
    return fail(AARMVS_ERR_INVALID, "cloud_nn: max_dist / cell exceeds AARMVS_CLOUD_MAX_RINGS");
  // other threads still read the inputs while a thread writes its outputs
  const size_t nq = (size_t)a->nq, m = (size_t)a->m;
  const void* outs[2] = {a->dist_out, a->index_out};
  for (int o = 0; o < 2; ++o) {
    if (!outs[o] || nq == 0) continue;
    if (ranges_overlap(outs[o], 4 * nq, a->query, 12 * nq) ||
        (m > 0 && (ranges_overlap(outs[o], 4 * nq, a->target, 12 * m) ||
                   ranges_overlap(outs[o], 4 * nq, a->target_keys, 8 * m) ||
                   (a->target_ids && ranges_overlap(outs[o], 4 * nq, a->target_ids, 4 * m)))))
      return fail(AARMVS_ERR_INVALID, o == 0 ? "cloud_nn: dist_out must not alias an input"
                                             : "cloud_nn: index_out must not alias an input");
  }
  if (nq > 0 && a->index_out && ranges_overlap(a->dist_out, 4 * nq, a->index_out, 4 * nq))
    return fail(AARMVS_ERR_INVALID, "cloud_nn: dist_out and index_out must not alias");
  return launched(launch_cloud_nn(a, stream), "cloud_nn");
}

size_t aarmvs_cloud_stats_scratch_bytes(long long n) {
  return cloud_count_ok(n) ? cloud_stats_scratch_bytes(n) : 0;
}

int aarmvs_cloud_stats(const float* dist, long long n, const float* thresholds, int n_thresholds, double* out,
                       void* scratch, hipStream_t stream) {
  if (!cloud_count_ok(n)) return fail(AARMVS_ERR_INVALID, "cloud_stats: need 0 <= n < 2^31");
  if (n_thresholds < 0 || n_thresholds > AARMVS_MAX_THRESHOLDS)
    return fail(AARMVS_ERR_INVALID, "cloud_stats: at most 8 thresholds");
  if (!out || !scratch || (n > 0 && !dist) || (n_thresholds > 0 && !thresholds))
    return fail(AARMVS_ERR_INVALID, "cloud_stats: null pointer argument");
  // blocks still read dist while others write their partials, and the reduce writes out after
  const size_t out_bytes = (3 + (size_t)n_thresholds) * sizeof(double), scr = cloud_stats_scratch_bytes(n);
  if (n > 0 && (ranges_overlap(out, out_bytes, dist, 4 * (size_t)n) || ranges_overlap(scratch, scr, dist, 4 * (size_t)n)))
    return fail(AARMVS_ERR_INVALID, "cloud_stats: out and scratch must not alias dist");
  if (ranges_overlap(out, out_bytes, scratch, scr))
    return fail(AARMVS_ERR_INVALID, "cloud_stats: out must not alias scratch");
  return launched(launch_cloud_stats(dist, n, thresholds, n_thresholds, out, scratch, stream), "cloud_stats");
}

size_t aarmvs_cloud_voxel_workspace_bytes(long long n) {
  return cloud_count_ok(n) ? cloud_voxel_workspace_bytes(n) : 0;
}

int aarmvs_cloud_voxel_centroids(const float* sorted_xyz, const long long* sorted_keys, long long n,
                                 float* out_xyz, long long capacity, long long* count, void* workspace,
                                 hipStream_t stream) {
  if (!cloud_count_ok(n)) return fail(AARMVS_ERR_INVALID, "cloud_voxel_centroids: need 0 <= n < 2^31");
  if (capacity < 0) return fail(AARMVS_ERR_INVALID, "cloud_voxel_centroids: negative capacity");
  if (!count || !workspace || (n > 0 && (!sorted_xyz || !sorted_keys)))
    return fail(AARMVS_ERR_INVALID, "cloud_voxel_centroids: null pointer argument");
  if (capacity > 0 && !out_xyz)
    return fail(AARMVS_ERR_INVALID, "cloud_voxel_centroids: null out_xyz with capacity > 0");
  if (n > 0 && capacity > 0 &&
      (ranges_overlap(out_xyz, 12 * (size_t)capacity, sorted_xyz, 12 * (size_t)n) ||
       ranges_overlap(out_xyz, 12 * (size_t)capacity, sorted_keys, 8 * (size_t)n)))
    return fail(AARMVS_ERR_INVALID, "cloud_voxel_centroids: out_xyz must not alias an input");
  return launched(launch_cloud_voxel_centroids(sorted_xyz, sorted_keys, n, out_xyz, capacity, count, workspace,
                                               stream),
                  "cloud_voxel_centroids");
}

size_t aarmvs_cloud_thin_scratch_bytes(long long n) {
  return cloud_count_ok(n) ? cloud_thin_scratch_bytes(n) : 0;
}

int aarmvs_cloud_thin(const aarmvs_cloud_thin_args* a, int rounds, hipStream_t stream) {
  if (!a) return fail(AARMVS_ERR_INVALID, "cloud_thin: null args");
  if (!cloud_count_ok(a->n)) return fail(AARMVS_ERR_INVALID, "cloud_thin: need 0 <= n < 2^31");
  if (rounds < 1) return fail(AARMVS_ERR_INVALID, "cloud_thin: need rounds >= 1");
  if (a->which != 0 && a->which != 1) return fail(AARMVS_ERR_INVALID, "cloud_thin: which must be 0 or 1");
  if (!a->remaining || !a->scratch ||
      (a->n > 0 && (!a->xyz || !a->keys || !a->rank || !a->state[0] || !a->state[1])))
    return fail(AARMVS_ERR_INVALID, "cloud_thin: null pointer argument");
  if (!cloud_origin_ok(a->origin)) return fail(AARMVS_ERR_INVALID, "cloud_thin: origin must be finite");
  if (!cloud_cell_ok(a->cell)) return fail(AARMVS_ERR_INVALID, "cloud_thin: cell must be finite and > 0");
  if (!(a->r >= 0.0f) || std::isinf(a->r)) return fail(AARMVS_ERR_INVALID, "cloud_thin: r must be finite and >= 0");
  if (a->cell < (double)a->r) return fail(AARMVS_ERR_INVALID, "cloud_thin: cell must be >= r");
  // a round's threads read the inputs and one state while others write the other state; the
  // per-block values and `remaining` are written between the rounds' reads
  const size_t n = (size_t)a->n, scr = cloud_thin_scratch_bytes(a->n);
  const void* outs[4] = {a->state[0], a->state[1], a->remaining, a->scratch};
  const size_t out_bytes[4] = {n, n, 2 * sizeof(long long), scr};
  const void* ins[3] = {a->xyz, a->keys, a->rank};
  const size_t in_bytes[3] = {12 * n, 8 * n, 4 * n};
  for (int o = 0; o < 4; ++o) {
    if (out_bytes[o] == 0) continue;
    for (int i = 0; i < 3; ++i)
      if (in_bytes[i] > 0 && ranges_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i]))
        return fail(AARMVS_ERR_INVALID, "cloud_thin: an output must not alias an input");
    for (int p = o + 1; p < 4; ++p)
      if (out_bytes[p] > 0 && ranges_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p]))
        return fail(AARMVS_ERR_INVALID, "cloud_thin: the outputs must not alias each other");
  }
  return launched(launch_cloud_thin(a, rounds, stream), "cloud_thin");
}

int aarmvs_cloud_regions(const float* xyz, long long n, const unsigned char* mask, const int* dims,
                         const double* bb, double res, double patch, const double* plane,
                         unsigned char* flags_out, hipStream_t stream) {
  if (!cloud_count_ok(n)) return fail(AARMVS_ERR_INVALID, "cloud_regions: need 0 <= n < 2^31");
  if ((n > 0 && (!xyz || !flags_out)) || (mask && (!bb || !dims)))
    return fail(AARMVS_ERR_INVALID, "cloud_regions: null pointer argument");
  if (bb)
    for (int k = 0; k < 6; ++k)
      if (!std::isfinite(bb[k])) return fail(AARMVS_ERR_INVALID, "cloud_regions: bb must be finite");
  if (!(patch >= 0.0) || std::isinf(patch))
    return fail(AARMVS_ERR_INVALID, "cloud_regions: patch must be finite and >= 0");
  size_t voxels = 0;
  if (mask) {
    if (!(res > 0.0) || std::isinf(res)) return fail(AARMVS_ERR_INVALID, "cloud_regions: res must be finite and > 0");
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1)
      return fail(AARMVS_ERR_INVALID, "cloud_regions: every mask dimension must be >= 1");
    voxels = 1;
    for (int k = 0; k < 3; ++k) {
      voxels *= (size_t)dims[k];                      // each factor < 2^31: no overflow before the test
      if (voxels >= ((size_t)1 << 31)) return fail(AARMVS_ERR_INVALID, "cloud_regions: the mask has 2^31 voxels or more");
    }
  }
  if (n > 0 && (ranges_overlap(flags_out, (size_t)n, xyz, 12 * (size_t)n) ||
                (mask && ranges_overlap(flags_out, (size_t)n, mask, voxels))))
    return fail(AARMVS_ERR_INVALID, "cloud_regions: flags_out must not alias an input");
  return launched(launch_cloud_regions(xyz, n, mask, dims, bb, res, patch, plane, flags_out, stream),
                  "cloud_regions");
}

}  // extern "C"
