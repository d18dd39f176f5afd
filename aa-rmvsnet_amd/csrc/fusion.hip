// Depth-map fusion core (fusion.py:71-220) for gfx950: per reference pixel, the geometric
// consistency against every source view's depth map (reproject_with_depth +
// check_geometric_consistency) and filter_depth's vote / mask / averaged-depth logic, in
// one pass (one thread per reference pixel, the source views in a loop).
//
// Arithmetic follows the reference's numpy types: projections in float64 on the float32
// camera matrices (the host packs them exactly as numpy forms them: float32 inverses and
// float32 matrix products), the maps, the reprojected depth and coordinates rounded to
// float32 where the reference casts, cv2.remap's INTER_LINEAR as OpenCV computes it for
// float maps (coordinates rounded to 1/32 px, table weights, left-to-right float32 sum,
// out-of-image taps 0), relative depth differences and depth sums in float32.
// Algorithmic bytes per reference pixel: depth + confidence (8) + one depth read per source
// view (4 nsrc) + three masks and the float64 average (11).  The de-duplicating instantiation
// (aarmvs_fusion_filter_dedup) adds the reference view's used byte and the emit mask (2) and one
// byte store per final pixel and consistent source view.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "aarmvs_internal.h"

namespace aarmvs {

struct FusionArgs {
  int H, W, nsrc;
  const float* ref_depth;
  const float* confidence;
  const float* src_depth[AARMVS_MAX_FUSION_SRC];
  float cams[AARMVS_FUSION_CAM_FLOATS(AARMVS_MAX_FUSION_SRC)];
  float photo_threshold;
  unsigned char* photo_mask;
  unsigned char* geo_mask;
  unsigned char* final_mask;
  double* depth_avg;
};

// the de-duplicating instantiation's arguments: the plain ones, then aarmvs_fusion_dedup_args
struct FusionDedupArgs : FusionArgs {
  const unsigned char* used_ref;
  unsigned char* used_src[AARMVS_MAX_FUSION_SRC];
  unsigned char* emit_mask;
};

// rows r of a row-major float32 matrix (columns cols) times a float64 vector, as numpy's
// float64 matmul of the up-cast matrix (an fma chain over k)
template <int COLS>
__device__ __forceinline__ double mrow(const float* m, int r, const double (&v)[COLS]) {
  double s = (double)m[r * COLS] * v[0];
#pragma unroll
  for (int k = 1; k < COLS; ++k) s = fma((double)m[r * COLS + k], v[k], s);
  return s;
}

// cv2.remap(src, map_x, map_y, INTER_LINEAR) at one pixel (BORDER_CONSTANT 0)
__device__ __forceinline__ float remap_linear(const float* __restrict__ src, int H, int W, float mx,
                                              float my) {
  auto to_fixed = [](float v) -> long long {
    const float t = __fmul_rn(v, 32.0f);
    // cvRound: nearest, ties to even; non-finite / out-of-int range -> INT_MIN (outside)
    if (!(fabsf(t) < 2147483520.0f)) return -2147483648LL;
    return (long long)rintf(t);
  };
  const long long X = to_fixed(mx), Y = to_fixed(my);
  const long long sx = X >> 5, sy = Y >> 5;
  const float fx = (float)(X & 31) * (1.0f / 32.0f), fy = (float)(Y & 31) * (1.0f / 32.0f);
  const float cx0 = __fsub_rn(1.0f, fx), cy0 = __fsub_rn(1.0f, fy);
  const float w0 = __fmul_rn(cy0, cx0), w1 = __fmul_rn(cy0, fx), w2 = __fmul_rn(fy, cx0),
              w3 = __fmul_rn(fy, fx);
  auto tap = [&](long long yy, long long xx) {
    return (xx >= 0 && xx < W && yy >= 0 && yy < H) ? src[yy * W + xx] : 0.0f;
  };
  float r = __fmul_rn(tap(sy, sx), w0);
  r = __fadd_rn(r, __fmul_rn(tap(sy, sx + 1), w1));
  r = __fadd_rn(r, __fmul_rn(tap(sy + 1, sx), w2));
  r = __fadd_rn(r, __fmul_rn(tap(sy + 1, sx + 1), w3));
  return r;
}

// DEDUP = false is the plain filter.  DEDUP = true (the visibility de-duplication,
// include/aarmvs.h): per source view, the pixel nearest to the float32 coordinates remap_linear
// is given -- or -1 where the i = 10 mask fails or that pixel lies outside the image -- waits in
// the thread's own LDS slots (an array indexed by the source view must not live in registers)
// until final is known; then emit = final && !used_ref is written, and a final pixel sets those
// pixels in the source views' used maps.  used_ref is only read and the used_src maps are only
// written here, and every writer stores 1.
template <bool DEDUP>
__global__ void __launch_bounds__(256)
fusion_filter_kernel(std::conditional_t<DEDUP, FusionDedupArgs, FusionArgs> a) {
  const int H = a.H, W = a.W, nsrc = a.nsrc, n = nsrc + 1;
  // cams: invK_ref[9], K_ref[9], then per source view K[9], invK[9], M1[12] = (E_src
  // inv(E_ref))[:3], M2[12] = (E_ref inv(E_src))[:3]
  const float* invK_ref = a.cams;
  const float* K_ref = a.cams + 9;
  [[maybe_unused]] int* marks = nullptr;   // [source view][thread]: nobody reads another's slot
  if constexpr (DEDUP) {
    __shared__ int mark_slots[AARMVS_MAX_FUSION_SRC * 256];
    marks = mark_slots + threadIdx.x;
  }
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < H * W; p += gridDim.x * blockDim.x) {
    const int y = p / W, x = p - y * W;
    const float dref = a.ref_depth[p];
    const double dd = (double)dref;
    const double b0[3] = {(double)x * dd, (double)y * dd, dd};
    const double xr[4] = {mrow<3>(invK_ref, 0, b0), mrow<3>(invK_ref, 1, b0), mrow<3>(invK_ref, 2, b0),
                          1.0};
    int votes[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int geo_sum = 0;
    float depth_sum = 0.0f;
    for (int v = 0; v < nsrc; ++v) {
      const float* c = a.cams + 18 + 42 * v;
      const float *K = c, *invK = c + 9, *M1 = c + 18, *M2 = c + 30;
      // step 1: reference pixel -> source view (fusion.py:75-87)
      const double xs3[3] = {mrow<4>(M1, 0, xr), mrow<4>(M1, 1, xr), mrow<4>(M1, 2, xr)};
      const double kx = mrow<3>(K, 0, xs3), ky = mrow<3>(K, 1, xs3), kz = mrow<3>(K, 2, xs3);
      const double xsrc = kx / kz, ysrc = ky / kz;
      // step 2: source depth at that point, back to the reference view (:89-108)
      const float sampled = remap_linear(a.src_depth[v], H, W, (float)xsrc, (float)ysrc);
      const double sd = (double)sampled;
      const double b2[3] = {xsrc * sd, ysrc * sd, sd};
      const double xs2[4] = {mrow<3>(invK, 0, b2), mrow<3>(invK, 1, b2), mrow<3>(invK, 2, b2), 1.0};
      const double xq[3] = {mrow<4>(M2, 0, xs2), mrow<4>(M2, 1, xs2), mrow<4>(M2, 2, xs2)};
      float depth_rep = (float)xq[2];
      const double qx = mrow<3>(K_ref, 0, xq), qy = mrow<3>(K_ref, 1, xq), qz = mrow<3>(K_ref, 2, xq);
      const float xrep = (float)(qx / qz), yrep = (float)(qy / qz);
      // check_geometric_consistency (:117-131)
      const double ex = (double)xrep - (double)x, ey = (double)yrep - (double)y;
      const double dist = sqrt(ex * ex + ey * ey);
      const float rel = __fdiv_rn(fabsf(__fsub_rn(depth_rep, dref)), dref);
      bool m = false;
#pragma unroll
      for (int i = 2; i <= 10; ++i) {
        m = dist < (double)i / 4.0 && rel < (float)((double)i / 1300.0);
        if (i < n) votes[i - 2] += m ? 1 : 0;   // filter_depth counts masks[0 .. n-3]
      }
      if (!m) depth_rep = 0.0f;   // depth_reprojected[~mask] = 0 (mask: i = 10)
      geo_sum += m ? 1 : 0;
      if constexpr (DEDUP) {
        // nearest pixel, ties to even; NaN and +-inf fail the comparisons
        const double X = (double)rintf((float)xsrc), Y = (double)rintf((float)ysrc);
        const bool inside = X >= 0.0 && X < (double)W && Y >= 0.0 && Y < (double)H;
        marks[v * 256] = (m && inside) ? (int)Y * W + (int)X : -1;
      }
      depth_sum = __fadd_rn(depth_sum, depth_rep);
    }
    // filter_depth (:207-220)
    bool geo = geo_sum >= n;
#pragma unroll
    for (int i = 2; i <= 10; ++i)
      if (i < n) geo = geo || votes[i - 2] >= i;
    const bool photo = a.confidence[p] > a.photo_threshold;
    a.photo_mask[p] = photo ? 1 : 0;
    a.geo_mask[p] = geo ? 1 : 0;
    a.final_mask[p] = (photo && geo) ? 1 : 0;
    a.depth_avg[p] = (double)__fadd_rn(depth_sum, dref) / (double)(geo_sum + 1);
    if constexpr (DEDUP) {
      const bool fin = photo && geo;
      const bool used = a.used_ref != nullptr && a.used_ref[p] != 0;
      a.emit_mask[p] = (fin && !used) ? 1 : 0;
      if (!fin) continue;
      for (int v = 0; v < nsrc; ++v) {
        unsigned char* mark = a.used_src[v];
        const int at = marks[v * 256];
        if (at >= 0 && mark != nullptr) mark[at] = 1;
      }
    }
  }
}

static int fusion_blocks(int H, int W) {
  return std::max(1, std::min((H * W + 255) / 256, 65535));
}

static void fill_fusion_args(FusionArgs& a, const aarmvs_fusion_args* in) {
  a.H = in->H;
  a.W = in->W;
  a.nsrc = in->nsrc;
  a.ref_depth = in->ref_depth;
  a.confidence = in->confidence;
  for (int v = 0; v < in->nsrc; ++v) a.src_depth[v] = in->src_depth[v];
  for (int i = 0; i < AARMVS_FUSION_CAM_FLOATS(in->nsrc); ++i) a.cams[i] = in->cams[i];
  a.photo_threshold = in->photo_threshold;
  a.photo_mask = in->photo_mask;
  a.geo_mask = in->geo_mask;
  a.final_mask = in->final_mask;
  a.depth_avg = in->depth_avg;
}

static hipError_t launch_fusion_filter(const aarmvs_fusion_args* in, hipStream_t s) {
  FusionArgs a{};
  fill_fusion_args(a, in);
  ProfScope ps(s, K_FUSION);
  hipLaunchKernelGGL(fusion_filter_kernel<false>, dim3(fusion_blocks(a.H, a.W)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// (timed under the plain filter's profile id: the list of kernel names is fixed)
static hipError_t launch_fusion_filter_dedup(const aarmvs_fusion_args* in, const aarmvs_fusion_dedup_args* d,
                                             hipStream_t s) {
  FusionDedupArgs a{};
  fill_fusion_args(a, in);
  a.used_ref = d->used_ref;
  for (int v = 0; v < in->nsrc; ++v) a.used_src[v] = d->used_src[v];
  a.emit_mask = d->emit_mask;
  ProfScope ps(s, K_FUSION);
  hipLaunchKernelGGL(fusion_filter_kernel<true>, dim3(fusion_blocks(a.H, a.W)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// cv2.pyrDown of the reference image (fusion_padding.py:166): OpenCV's scalar float path
// (imgproc/src/pyramids.cpp), every intermediate rounded to float32.  A block owns a tile of
// kPyrTY x kPyrTX output pixels: the horizontal pass of the 2 kPyrTY + 3 source rows it
// needs goes to LDS, the vertical pass reads it from there.
// Algorithmic bytes: 4 C (H W + H W / 4).
// ---------------------------------------------------------------------------------
constexpr int kPyrTX = 32, kPyrTY = 8, kPyrRows = 2 * kPyrTY + 3;

// BORDER_REFLECT_101 for i in [-2, n + 1], n >= 4
__device__ __forceinline__ int reflect101(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i;
}

// s0*6 + (sm1 + sp1)*4 + sm2 + sp2, summed left to right
__device__ __forceinline__ float pyr_taps(float sm2, float sm1, float s0, float sp1, float sp2) {
  float v = __fadd_rn(__fmul_rn(s0, 6.0f), __fmul_rn(__fadd_rn(sm1, sp1), 4.0f));
  v = __fadd_rn(v, sm2);
  return __fadd_rn(v, sp2);
}

template <int C>
__global__ void __launch_bounds__(256) pyr_down_kernel(const float* __restrict__ src, int H, int W,
                                                       float* __restrict__ dst, int Ho, int Wo) {
  constexpr int RW = kPyrTX * C;
  __shared__ float r[kPyrRows][RW];
  const int x0 = blockIdx.x * kPyrTX, y0 = blockIdx.y * kPyrTY;
  for (int j = threadIdx.x; j < kPyrRows * RW; j += 256) {
    const int rr = j / RW, xc = j - rr * RW;
    const int xo = x0 + xc / C, c = xc % C;
    const int sy = 2 * y0 - 2 + rr;
    // rows past 2 Ho and columns past Wo feed no output of this image (and lie beyond what
    // the border rule covers)
    if (sy > 2 * Ho || xo >= Wo) continue;
    const float* s = src + (size_t)reflect101(sy, H) * W * C + c;
    const int sx = 2 * xo;
    r[rr][xc] = pyr_taps(s[reflect101(sx - 2, W) * C], s[reflect101(sx - 1, W) * C], s[sx * C],
                         s[reflect101(sx + 1, W) * C], s[reflect101(sx + 2, W) * C]);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < kPyrTY * RW; j += 256) {
    const int ty = j / RW, xc = j - ty * RW;
    const int yo = y0 + ty, xo = x0 + xc / C;
    if (yo >= Ho || xo >= Wo) continue;
    const float v = pyr_taps(r[2 * ty][xc], r[2 * ty + 1][xc], r[2 * ty + 2][xc], r[2 * ty + 3][xc],
                             r[2 * ty + 4][xc]);
    dst[((size_t)yo * Wo + x0) * C + xc] = __fmul_rn(v, 1.0f / 256.0f);
  }
}

static hipError_t launch_pyr_down(const float* src, int H, int W, int C, float* dst, hipStream_t s) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const dim3 grid((Wo + kPyrTX - 1) / kPyrTX, (Ho + kPyrTY - 1) / kPyrTY);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  ProfScope ps(s, K_PYR_DOWN);
  if (C == 3)
    hipLaunchKernelGGL(pyr_down_kernel<3>, grid, dim3(256), 0, s, src, H, W, dst, Ho, Wo);
  else
    hipLaunchKernelGGL(pyr_down_kernel<1>, grid, dim3(256), 0, s, src, H, W, dst, Ho, Wo);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// World points of the kept pixels, in pixel order (fusion.py:235-246,
// fusion_padding.py:239-251).  A block owns kPtsChunk consecutive pixels, taken in
// kPtsRounds rounds of one pixel per thread.  Three launches: the kept pixels of every block,
// an exclusive scan of those counts by one workgroup (tile after tile, with a carry), and the
// write pass, where a pixel's rank is its block's offset + the kept pixels of the block's
// earlier (round, wave) groups + the set ballot bits below its lane.
// Algorithmic bytes: 1 per pixel + (8 depth + 12 colour + 12 xyz + 3 rgb) per kept pixel.
// ---------------------------------------------------------------------------------
constexpr int kPtsThreads = 256, kPtsRounds = 4, kPtsWaves = kPtsThreads / 64;
constexpr int kPtsChunk = kPtsThreads * kPtsRounds;
constexpr int kScanThreads = 256;   // block counts per scan tile

struct PointsArgs {
  int HW, W;
  const unsigned char* mask;
  const double* depth;
  const float* color;
  float invK[9], invE[16];
  float* xyz;
  unsigned char* rgb;
  long long capacity;
  const int* block_off;
};

// the instantiation with normals (aarmvs_fusion_points_normals): the plain arguments, then the
// view's normal map and the kept pixels' normals
struct PointsNormalsArgs : PointsArgs {
  const float* normal_map;
  float* nxyz;
};

__global__ void __launch_bounds__(kPtsThreads) points_count_kernel(const unsigned char* __restrict__ mask,
                                                                   int HW, int* __restrict__ block_cnt) {
  __shared__ int wcnt[kPtsWaves];
  const long long base = (long long)blockIdx.x * kPtsChunk;
  int c = 0;
#pragma unroll
  for (int r = 0; r < kPtsRounds; ++r) {
    const long long p = base + r * kPtsThreads + threadIdx.x;
    const bool keep = p < HW && mask[p] != 0;
    c += __popcll(__ballot(keep));
  }
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kPtsWaves; ++w) t += wcnt[w];
    block_cnt[blockIdx.x] = t;
  }
}

// cnt[0 .. n) -> its exclusive prefix sums, in place; *total = the sum (< 2^31: H W is)
__global__ void __launch_bounds__(kScanThreads) points_scan_kernel(int* __restrict__ cnt, int n,
                                                                   long long* __restrict__ total) {
  __shared__ int wsum[kScanThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += kScanThreads) {
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
    for (int w = 0; w < kScanThreads / 64; ++w) {
      before += w < wave ? wsum[w] : 0;
      tile += wsum[w];
    }
    if (i < n) cnt[i] = carry + before + s - v;
    carry += tile;
    __syncthreads();   // wsum is rewritten by the next tile
  }
  if (threadIdx.x == 0) *total = carry;
}

// NORMALS = false is the plain write pass.  NORMALS = true also copies the kept pixel's normal to
// its rank: nxyz lines up with xyz and rgb.
template <bool NORMALS>
__global__ void __launch_bounds__(kPtsThreads)
points_write_kernel(std::conditional_t<NORMALS, PointsNormalsArgs, PointsArgs> a) {
  __shared__ int wcnt[kPtsRounds][kPtsWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * kPtsChunk;
  bool keep[kPtsRounds];
  int below[kPtsRounds];
#pragma unroll
  for (int r = 0; r < kPtsRounds; ++r) {
    const long long p = base + r * kPtsThreads + threadIdx.x;
    keep[r] = p < a.HW && a.mask[p] != 0;
    const unsigned long long b = __ballot(keep[r]);
    below[r] = __popcll(b & ((1ULL << lane) - 1ULL));
    if (lane == 0) wcnt[r][wave] = __popcll(b);
  }
  __syncthreads();
  long long acc = a.block_off[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kPtsRounds; ++r) {
    int before = 0, round = 0;
#pragma unroll
    for (int w = 0; w < kPtsWaves; ++w) {
      before += w < wave ? wcnt[r][w] : 0;
      round += wcnt[r][w];
    }
    const long long rank = acc + before + below[r];
    acc += round;
    if (!keep[r] || rank >= a.capacity) continue;
    const int p = (int)(base + r * kPtsThreads + threadIdx.x);
    const int y = p / a.W, x = p - y * a.W;
    const double d = a.depth[p];
    const double b[3] = {(double)x * d, (double)y * d, d};
    const double xr[4] = {mrow<3>(a.invK, 0, b), mrow<3>(a.invK, 1, b), mrow<3>(a.invK, 2, b), 1.0};
    float* o = a.xyz + (size_t)rank * 3;
    o[0] = (float)mrow<4>(a.invE, 0, xr);
    o[1] = (float)mrow<4>(a.invE, 1, xr);
    o[2] = (float)mrow<4>(a.invE, 2, xr);
    if (a.color) {
      const float* c = a.color + (size_t)p * 3;
      unsigned char* q = a.rgb + (size_t)rank * 3;
      q[0] = (unsigned char)(int)__fmul_rn(c[0], 255.0f);
      q[1] = (unsigned char)(int)__fmul_rn(c[1], 255.0f);
      q[2] = (unsigned char)(int)__fmul_rn(c[2], 255.0f);
    }
    if constexpr (NORMALS) {
      const float* nm = a.normal_map + (size_t)p * 3;
      float* no = a.nxyz + (size_t)rank * 3;
      no[0] = nm[0];
      no[1] = nm[1];
      no[2] = nm[2];
    }
  }
}

static int points_blocks(int H, int W) {
  return (int)(((long long)H * W + kPtsChunk - 1) / kPtsChunk);
}

static size_t fusion_points_workspace_bytes(int H, int W) {
  return ((size_t)points_blocks(H, W) * sizeof(int) + 255) / 256 * 256;
}

// normal_map == nullptr: the plain write pass (nxyz is not looked at)
static hipError_t launch_fusion_points(const aarmvs_fusion_points_args* in, const float* normal_map, float* nxyz,
                                       hipStream_t s) {
  PointsNormalsArgs a{};
  a.HW = in->H * in->W;
  a.W = in->W;
  a.mask = in->mask;
  a.depth = in->depth;
  a.color = in->color;
  for (int i = 0; i < 9; ++i) a.invK[i] = in->cams[i];
  for (int i = 0; i < 16; ++i) a.invE[i] = in->cams[9 + i];
  a.xyz = in->xyz;
  a.rgb = in->rgb;
  a.capacity = in->capacity;
  int* blk = static_cast<int*>(in->workspace);
  a.block_off = blk;
  const int nb = points_blocks(in->H, in->W);
  ProfScope ps(s, K_FUSION_POINTS);
  hipLaunchKernelGGL(points_count_kernel, dim3(nb), dim3(kPtsThreads), 0, s, a.mask, a.HW, blk);
  hipLaunchKernelGGL(points_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, blk, nb, in->count);
  if (normal_map != nullptr) {
    a.normal_map = normal_map;
    a.nxyz = nxyz;
    hipLaunchKernelGGL(points_write_kernel<true>, dim3(nb), dim3(kPtsThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL(points_write_kernel<false>, dim3(nb), dim3(kPtsThreads), 0, s,
                       static_cast<const PointsArgs&>(a));
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Per-pixel normals of a view's averaged depth map (aarmvs_fusion_normals, include/aarmvs.h): a
// least-squares fit of 1/d = a x + b y + c over the usable pixels of a (2R+1)^2 window, in float64
// with every operation rounded on its own and the sums in the header's order.  A block owns a
// kNrmTY x kNrmTX tile: the depth of the tile and its R-wide halo goes to LDS once -- NaN where a
// pixel is not usable or outside the image, which fails the per-tap gate by itself -- beside its
// reciprocal, computed once per pixel.  A wave owns a tile row at a time, so its 8-byte LDS reads
// are 64 consecutive doubles.  No atomics; the only global reads are the bounds-checked tile loads.
// Algorithmic bytes per pixel: 9 read (+ halo) and 12 or 13 written.
// ---------------------------------------------------------------------------------
constexpr int kNrmTX = 64, kNrmTY = 16, kNrmThreads = 256;

struct NormalsArgs {
  int H, W, tiles_x, min_count;
  const double* depth;
  const unsigned char* valid;
  float K[9], R[9];   // K, and the upper-left 3x3 of inv(E)
  double max_rel_jump;
  float* normal;
  unsigned char* has_normal;
};

template <int R>
__global__ void __launch_bounds__(kNrmThreads) fusion_normals_kernel(NormalsArgs a) {
  constexpr int LH = kNrmTY + 2 * R, LW = kNrmTX + 2 * R;
  __shared__ double sd[LH][LW];   // the depth of a usable pixel, else NaN
  __shared__ double sw[LH][LW];   // 1 / sd
  const int by = blockIdx.x / a.tiles_x, bx = blockIdx.x - by * a.tiles_x;
  const int x_tile = bx * kNrmTX, y_tile = by * kNrmTY;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int j = threadIdx.x; j < LH * LW; j += kNrmThreads) {
    const int ly = j / LW, lx = j - ly * LW;
    const int gy = y_tile - R + ly, gx = x_tile - R + lx;
    double d = nan;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const size_t q = (size_t)gy * a.W + gx;
      const double t = a.depth[q];
      if (a.valid[q] != 0 && t > 0.0 && t < __longlong_as_double(0x7ff0000000000000LL)) d = t;
    }
    sd[ly][lx] = d;
    sw[ly][lx] = __ddiv_rn(1.0, d);
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = x_tile + tx;
  if (x0 >= a.W) return;
#pragma unroll 1
  for (int k = 0; k < kNrmTY / 4; ++k) {
    const int ty = wave + 4 * k, y0 = y_tile + ty;
    if (y0 >= a.H) break;
    const size_t p = (size_t)y0 * a.W + x0;
    const double d0 = sd[ty + R][tx + R];
    const double lim = __dmul_rn(a.max_rel_jump, d0);
    int A = 0, B = 0, C = 0, D = 0, E = 0, N = 0;
    double Suw = 0.0, Svw = 0.0, Sw = 0.0;
#pragma unroll
    for (int v = -R; v <= R; ++v) {
#pragma unroll
      for (int u = -R; u <= R; ++u) {
        const double dq = sd[ty + R + v][tx + R + u];
        // NaN (the centre's or the neighbour's) fails the comparison
        if (fabs(__dsub_rn(dq, d0)) <= lim) {
          const double w = sw[ty + R + v][tx + R + u];
          A += u * u;
          B += u * v;
          C += v * v;
          D += u;
          E += v;
          N += 1;
          Suw = __dadd_rn(Suw, __dmul_rn((double)u, w));
          Svw = __dadd_rn(Svw, __dmul_rn((double)v, w));
          Sw = __dadd_rn(Sw, w);
        }
      }
    }
    // cofactors of the normal matrix: exact integers (below 2^31 for R <= 3)
    const int c00 = C * N - E * E, c01 = D * E - B * N, c02 = B * E - C * D;
    const int c11 = A * N - D * D, c12 = B * D - A * E, c22 = A * C - B * B;
    const int det = (A * c00 + B * c01) + D * c02;
    auto dot3 = [](double k0, double v0, double k1, double v1, double k2, double v2) {
      return __dadd_rn(__dadd_rn(__dmul_rn(k0, v0), __dmul_rn(k1, v1)), __dmul_rn(k2, v2));
    };
    const double pa = dot3((double)c00, Suw, (double)c01, Svw, (double)c02, Sw);
    const double pb = dot3((double)c01, Suw, (double)c11, Svw, (double)c12, Sw);
    const double pc = dot3((double)c02, Suw, (double)c12, Svw, (double)c22, Sw);
    const double cabs = __dsub_rn(__dsub_rn(pc, __dmul_rn(pa, (double)x0)), __dmul_rn(pb, (double)y0));
    double m[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      m[i] = dot3((double)a.K[i], pa, (double)a.K[3 + i], pb, (double)a.K[6 + i], cabs);
    const double len = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(m[0], m[0]), __dmul_rn(m[1], m[1])),
                                      __dmul_rn(m[2], m[2])));
    // (a NaN centre gathers nothing: N = 0)
    const bool has = N >= a.min_count && det > 0 && len > 0.0 &&
                     len < __longlong_as_double(0x7ff0000000000000LL);
    float out[3] = {0.0f, 0.0f, 0.0f};
    if (has) {
      const double n0 = -__ddiv_rn(m[0], len), n1 = -__ddiv_rn(m[1], len), n2 = -__ddiv_rn(m[2], len);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        out[i] = (float)dot3((double)a.R[3 * i], n0, (double)a.R[3 * i + 1], n1, (double)a.R[3 * i + 2], n2);
    }
    float* o = a.normal + p * 3;
    o[0] = out[0];
    o[1] = out[1];
    o[2] = out[2];
    if (a.has_normal != nullptr) a.has_normal[p] = has ? 1 : 0;
  }
}

// (timed under the points' profile id: the list of kernel names is fixed)
static hipError_t launch_fusion_normals(const aarmvs_fusion_normals_args* in, hipStream_t s) {
  NormalsArgs a{};
  a.H = in->H;
  a.W = in->W;
  a.tiles_x = (in->W + kNrmTX - 1) / kNrmTX;
  a.min_count = in->min_count;
  a.depth = in->depth;
  a.valid = in->valid;
  for (int i = 0; i < 9; ++i) a.K[i] = in->cams[i];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) a.R[3 * i + j] = in->cams[9 + 4 * i + j];
  a.max_rel_jump = (double)in->max_rel_jump;
  a.normal = in->normal;
  a.has_normal = in->has_normal;
  // H W < 2^31, so the tiles are fewer than 2^31 too
  const long long tiles = (long long)a.tiles_x * ((in->H + kNrmTY - 1) / kNrmTY);
  if (tiles >= (1LL << 31)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tiles), block(kNrmThreads);
  ProfScope ps(s, K_FUSION_POINTS);
  switch (in->radius) {
    case 1: hipLaunchKernelGGL(fusion_normals_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(fusion_normals_kernel<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(fusion_normals_kernel<3>, grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace aarmvs

using namespace aarmvs;

extern "C" {

static int fusion_filter_check(const aarmvs_fusion_args* a) {
  if (!a) return fail(AARMVS_ERR_INVALID, "fusion_filter: null args");
  if (a->H < 1 || a->W < 1 || a->nsrc < 1 || a->nsrc > AARMVS_MAX_FUSION_SRC)
    return fail(AARMVS_ERR_INVALID, "fusion_filter: need H, W >= 1 and 1 <= nsrc <= 10");
  if (!a->ref_depth || !a->confidence || !a->cams || !a->photo_mask || !a->geo_mask ||
      !a->final_mask || !a->depth_avg)
    return fail(AARMVS_ERR_INVALID, "fusion_filter: null pointer argument");
  for (int v = 0; v < a->nsrc; ++v)
    if (!a->src_depth[v]) return fail(AARMVS_ERR_INVALID, "fusion_filter: null src_depth pointer");
  return AARMVS_OK;
}

int aarmvs_fusion_filter(const aarmvs_fusion_args* a, hipStream_t stream) {
  if (int rc = fusion_filter_check(a)) return rc;
  return launched(launch_fusion_filter(a, stream), "fusion_filter");
}

int aarmvs_fusion_filter_dedup(const aarmvs_fusion_args* a, const aarmvs_fusion_dedup_args* d,
                               hipStream_t stream) {
  if (!d) return aarmvs_fusion_filter(a, stream);
  if (int rc = fusion_filter_check(a)) return rc;
  if (!d->emit_mask) return fail(AARMVS_ERR_INVALID, "fusion_filter_dedup: null emit_mask");
  if (d->emit_mask == a->photo_mask || d->emit_mask == a->geo_mask || d->emit_mask == a->final_mask)
    return fail(AARMVS_ERR_INVALID,
                "fusion_filter_dedup: emit_mask must not be the photo, geo or final mask");
  // a launch only reads used_ref and only writes the used_src maps: a view is not its own source
  for (int v = 0; v < a->nsrc; ++v)
    if (d->used_ref && d->used_src[v] == d->used_ref)
      return fail(AARMVS_ERR_INVALID, "fusion_filter_dedup: used_ref must not be one of used_src");
  return launched(launch_fusion_filter_dedup(a, d, stream), "fusion_filter_dedup");
}

int aarmvs_pyr_down(const float* src, int H, int W, int C, float* dst, hipStream_t stream) {
  if (!src || !dst) return fail(AARMVS_ERR_INVALID, "pyr_down: null pointer argument");
  if (H < 4 || W < 4 || (C != 1 && C != 3))
    return fail(AARMVS_ERR_INVALID, "pyr_down: need H, W >= 4 and C = 1 or 3");
  if ((long long)H * W * C >= (1LL << 31))
    return fail(AARMVS_ERR_INVALID, "pyr_down: H * W * C must be below 2^31");
  return launched(launch_pyr_down(src, H, W, C, dst, stream), "pyr_down");
}

size_t aarmvs_fusion_points_workspace_bytes(int H, int W) {
  if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) return 0;
  return fusion_points_workspace_bytes(H, W);
}

static int fusion_points_check(const aarmvs_fusion_points_args* a) {
  if (!a) return fail(AARMVS_ERR_INVALID, "fusion_points: null args");
  if (a->H < 1 || a->W < 1 || (long long)a->H * a->W >= (1LL << 31))
    return fail(AARMVS_ERR_INVALID, "fusion_points: need H, W >= 1 and H * W < 2^31");
  if (!a->mask || !a->depth || !a->cams || !a->count || !a->workspace)
    return fail(AARMVS_ERR_INVALID, "fusion_points: null pointer argument");
  if (a->capacity < 0) return fail(AARMVS_ERR_INVALID, "fusion_points: negative capacity");
  if (a->capacity > 0 && !a->xyz)
    return fail(AARMVS_ERR_INVALID, "fusion_points: null xyz with capacity > 0");
  if ((a->color == nullptr) != (a->rgb == nullptr))
    return fail(AARMVS_ERR_INVALID, "fusion_points: color and rgb must both be set or both be null");
  return AARMVS_OK;
}

int aarmvs_fusion_points(const aarmvs_fusion_points_args* a, hipStream_t stream) {
  if (int rc = fusion_points_check(a)) return rc;
  return launched(launch_fusion_points(a, nullptr, nullptr, stream), "fusion_points");
}

int aarmvs_fusion_points_normals(const aarmvs_fusion_points_args* a, const float* normal_map, float* nxyz,
                                 hipStream_t stream) {
  if (!normal_map && !nxyz) return aarmvs_fusion_points(a, stream);
  if (int rc = fusion_points_check(a)) return rc;
  if (!normal_map || !nxyz)
    return fail(AARMVS_ERR_INVALID,
                "fusion_points_normals: normal_map and nxyz must both be set or both be null");
  return launched(launch_fusion_points(a, normal_map, nxyz, stream), "fusion_points_normals");
}

int aarmvs_fusion_normals(const aarmvs_fusion_normals_args* a, hipStream_t stream) {
  if (!a) return fail(AARMVS_ERR_INVALID, "fusion_normals: null args");
  if (a->H < 1 || a->W < 1 || (long long)a->H * a->W >= (1LL << 31))
    return fail(AARMVS_ERR_INVALID, "fusion_normals: need H, W >= 1 and H * W < 2^31");
  if (!a->depth || !a->valid || !a->cams || !a->normal)
    return fail(AARMVS_ERR_INVALID, "fusion_normals: null pointer argument");
  if (a->radius < 1 || a->radius > AARMVS_MAX_NORMAL_RADIUS)
    return fail(AARMVS_ERR_INVALID, "fusion_normals: radius must be 1, 2 or 3");
  const int window = (2 * a->radius + 1) * (2 * a->radius + 1);
  if (a->min_count < 3 || a->min_count > window)
    return fail(AARMVS_ERR_INVALID, "fusion_normals: min_count must be in 3 .. (2 radius + 1)^2");
  if (!(a->max_rel_jump >= 0.0f) || std::isinf(a->max_rel_jump))
    return fail(AARMVS_ERR_INVALID, "fusion_normals: max_rel_jump must be finite and >= 0");
  // other blocks still read depth and valid while a block writes its outputs
  const size_t px = (size_t)a->H * a->W;
  if (ranges_overlap(a->normal, 12 * px, a->depth, 8 * px) || ranges_overlap(a->normal, 12 * px, a->valid, px))
    return fail(AARMVS_ERR_INVALID, "fusion_normals: normal must not alias depth or valid");
  if (a->has_normal &&
      (ranges_overlap(a->has_normal, px, a->depth, 8 * px) || ranges_overlap(a->has_normal, px, a->valid, px) ||
       ranges_overlap(a->has_normal, px, a->normal, 12 * px)))
    return fail(AARMVS_ERR_INVALID, "fusion_normals: has_normal must not alias depth, valid or normal");
  return launched(launch_fusion_normals(a, stream), "fusion_normals");
}

}  // extern "C"
