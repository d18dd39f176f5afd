// What the warp and cost-slice units share (warp.hip, cost_fwd.hip, cost_bwd.hip): the sampling
// position, the pipeline's argument struct, and the tap, omega-parameter and box helpers that
// the backward recomputes the forward with.  Everything here is used by more than one unit.
#pragma once

#include <climits>

#include "device_common.h"

namespace aarmvs {

// ---------------------------------------------------------------------------
// Sampling position of reference pixel (x, y) in the source view, in source
// pixel units, following module.py:26-33 then grid_sample's align_corners=False
// unnormalisation.  The grid itself is built by separate torch ops in the
// reference (explicit _rn ops here: no contraction); grid_sample's CPU kernel is
// FMA-contracted by its compiler: ix = fma(g + 1, size/2, -0.5).  This pair of
// choices reproduces the reference's sampling positions bit for bit.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void sample_pos(const float* __restrict__ m, float depth, float x,
                                           float y, int H, int W, float& ix, float& iy) {
  float p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float rx = __fadd_rn(__fadd_rn(__fmul_rn(m[4 * k + 0], x), __fmul_rn(m[4 * k + 1], y)),
                               m[4 * k + 2]);                     // rot @ [x,y,1]   :26
    p[k] = __fadd_rn(__fmul_rn(rx, depth), m[4 * k + 3]);         // * depth + t     :27-28
  }
  float z = p[2];
  if (z == 0.0f) z = __fadd_rn(z, 1e-4f);                         // :29
  const float px = __fdiv_rn(p[0], z), py = __fdiv_rn(p[1], z);   // :30
  const float gx = __fsub_rn(__fdiv_rn(px, (float)(W - 1) * 0.5f), 1.0f);  // :31
  const float gy = __fsub_rn(__fdiv_rn(py, (float)(H - 1) * 0.5f), 1.0f);  // :32
  ix = __fmaf_rn(__fadd_rn(gx, 1.0f), (float)W * 0.5f, -0.5f);
  iy = __fmaf_rn(__fadd_rn(gy, 1.0f), (float)H * 0.5f, -0.5f);
}

// bound on |k| of the fixed-point exponents (warp_bwd_exp, cbw_scale_kernel): 2^k is applied
// with ldexp on values whose scaled magnitude is <= 2^61, and removed in fp64
constexpr int kFixedExpMax = 250;

struct PipeArgs {
  const float* ref;
  const float* src[AARMVS_MAX_SRC];
  const float* rel;           // [nsrc][B][12]
  const float* dvals;         // [B][D]
  int D;
  int d_prev, d_next;         // -1: part disabled
  const float4* t1_prev;      // [B][nsrc][HW]
  float4* t1_next;
  const double* st_prev;      // [B][nsrc][3][kSlots][2]
  double* st_next;
  float* x;                   // [B,H,W,32] (NHWC)
  float* omega_out;           // [nsrc,B,H,W] (prev plane) or null
  const float* params;
  size_t off_owb_scale;            // the omega conv fragments' scale
  size_t off_owm, off_owm_scale;   // omega_mfma's 32x32x16 fragments, their scale
  size_t off_ow0t, off_ow0, off_ob0, off_og0w, off_og0b, off_ow1, off_ob1, off_og1w, off_og1b, off_ow2,
      off_ob2, off_og2w, off_og2b, off_owo, off_obo;
  int B, H, W, nsrc;
  int box_cap;                // LDS source-box capacity in pixels (diagnostic override, <= the kernel's)
  // plane batching: one launch covers planes d .. d + npl - 1 (d = d_prev or d_next), plane
  // k's t1 / statistics / x at k times these strides from the plane-0 pointers
  int npl;
  size_t t1_kstride;          // float4s
  size_t st_kstride;          // doubles
  size_t x_kstride;           // floats
  int omega_k;                // cost_x: the plane (0 .. npl-1) whose omega weights go to omega_out
  // GroupNorm partial sums: one (sum, sumsq) per producing block, [npl][B][nsrc][part_n],
  // reduced in a fixed order by stat_reduce_kernel (deterministic statistics, independent of
  // the launch's grouping and of block timing)
  double* part;
  int part_n;
  int omega_ipb;              // omega_mfma: planes per block (AARMVS_OMEGA_IPB, default 1)
};

// omega pointwise chain helpers (ResnetBlockGn, module.py:252-264)
struct OmegaP {
  float w1[16], b1[4], w2[16], b2[4], wo[4], bo;
  float g0w[4], g0b[4], g1w[4], g1b[4], g2w[4], g2b[4];
};

__device__ __forceinline__ void load_omega(const PipeArgs& a, const float* __restrict__ P,
                                           OmegaP& o) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    o.w1[i] = P[a.off_ow1 + i];
    o.w2[i] = P[a.off_ow2 + i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o.b1[i] = P[a.off_ob1 + i];
    o.b2[i] = P[a.off_ob2 + i];
    o.wo[i] = P[a.off_owo + i];
    o.g0w[i] = P[a.off_og0w + i];
    o.g0b[i] = P[a.off_og0b + i];
    o.g1w[i] = P[a.off_og1w + i];
    o.g1b[i] = P[a.off_og1b + i];
    o.g2w[i] = P[a.off_og2w + i];
    o.g2b[i] = P[a.off_og2b + i];
  }
  o.bo = P[a.off_obo];
}

__device__ __forceinline__ void conv1x1_4(const float (&x)[4], const float* w, const float* bias,
                                          float (&y)[4]) {
#pragma unroll
  for (int co = 0; co < 4; ++co) {
    float s = 0.f;
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) s = fmaf(w[co * 4 + ci], x[ci], s);
    y[co] = s + bias[co];
  }
}

__device__ __forceinline__ size_t st_index(int b, int v, int k, int nsrc) {
  return (((size_t)b * nsrc + v) * 3 + k) * kSlots * 2;
}

// omega_conv tiles are 32 pixels wide, 16 rows (one thread per pixel).
constexpr int kTileW = 32, kTileH = 16, kTileThreads = kTileW * kTileH;
constexpr int kTileWaves = kTileThreads / 64;

// XCD-aware tile order: blocks are dealt to the 8 XCDs round-robin, so XCD k takes the
// k-th contiguous band of tiles and neighbouring tiles (which share source rows) share
// its L2
__device__ __forceinline__ int xcd_tile(int bid, int nb) {
  const int q8 = nb >> 3, r8 = nb & 7, xcd = bid & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// A sampling position reduced to what the taps need: the top-left tap's floor
// coordinates and the four bilinear weights (make_taps' arithmetic).
struct TapF {
  float xf, yf;
  float wt[4];
};

__device__ __forceinline__ TapF tap_f(const float* __restrict__ m, float dep, int x, int y, int H,
                                      int W) {
  float ix, iy;
  sample_pos(m, dep, (float)x, (float)y, H, W, ix, iy);
  TapF t;
  t.xf = floorf(ix);
  t.yf = floorf(iy);
  const float wx = __fsub_rn(ix, t.xf), wy = __fsub_rn(iy, t.yf);
  const float ex = __fsub_rn(1.0f, wx), sy = __fsub_rn(1.0f, wy);
  t.wt[0] = __fmul_rn(sy, ex);
  t.wt[1] = __fmul_rn(sy, wx);
  t.wt[2] = __fmul_rn(wy, ex);
  t.wt[3] = __fmul_rn(wy, wx);
  return t;
}

struct Box {
  int x0, y0, nx, ny;
};

// red: LDS scratch [NW][4] (NW: the block's waves); must not be read by anyone before the
// barrier here
template <int NW = kTileWaves>
__device__ __forceinline__ Box box_reduce(int lx, int ly, int hx, int hy, int (*red)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  auto mn = [](int a, int b) { return min(a, b); };
  auto mx = [](int a, int b) { return max(a, b); };
  lx = wave_reduce_i32(lx, INT_MAX, mn);
  ly = wave_reduce_i32(ly, INT_MAX, mn);
  hx = wave_reduce_i32(hx, INT_MIN, mx);
  hy = wave_reduce_i32(hy, INT_MIN, mx);
  if (lane == 0) {
    red[wave][0] = lx;
    red[wave][1] = ly;
    red[wave][2] = hx;
    red[wave][3] = hy;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    lx = min(lx, red[w][0]);
    ly = min(ly, red[w][1]);
    hx = max(hx, red[w][2]);
    hy = max(hy, red[w][3]);
  }
  Box bx;
  bx.x0 = __builtin_amdgcn_readfirstlane(lx);
  bx.y0 = __builtin_amdgcn_readfirstlane(ly);
  bx.nx = __builtin_amdgcn_readfirstlane(hx >= lx ? hx - lx + 1 : 0);
  bx.ny = __builtin_amdgcn_readfirstlane(hy >= ly ? hy - ly + 1 : 0);
  return bx;
}

// The four taps of a position: pixel indices (into the LDS box, or image pixels for
// the global path) and weights; out-of-image taps get `zpix` (the box's zero pixel, or
// a pixel index whose byte offset lies past the buffer: loads 0).
struct TapP {
  uint32_t pix[4];
  float wt[4];
};

__device__ __forceinline__ TapP tap_p(const TapF& t, bool valid, int H, int W, bool lds,
                                      const Box& bx, uint32_t zpix) {
  TapP o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o.wt[k] = t.wt[k];
    const float xf = t.xf + (float)(k & 1), yf = t.yf + (float)(k >> 1);
    const bool ok = valid && (xf > -1.0f) && (xf < (float)W) && (yf > -1.0f) && (yf < (float)H);
    const int xi = ok ? (int)xf : bx.x0, yi = ok ? (int)yf : bx.y0;
    // 24-bit multiplies (full rate): coordinates and extents are < 2^24
    const uint32_t p = lds ? __umul24((uint32_t)(yi - bx.y0), (uint32_t)bx.nx) + (uint32_t)(xi - bx.x0)
                           : __umul24((uint32_t)yi, (uint32_t)W) + (uint32_t)xi;
    o.pix[k] = ok ? p : zpix;
  }
  return o;
}

__device__ __forceinline__ float bil1(float v0, float v1, float v2, float v3, const TapP& t) {
  return __fmaf_rn(v3, t.wt[3], __fmaf_rn(v2, t.wt[2], __fmaf_rn(v1, t.wt[1], __fmul_rn(v0, t.wt[0]))));
}

// the fma chain of bilinear() on 4 channels
__device__ __forceinline__ float4 bil4(float4 v0, float4 v1, float4 v2, float4 v3, const TapP& t) {
  return make_float4(bil1(v0.x, v1.x, v2.x, v3.x, t), bil1(v0.y, v1.y, v2.y, v3.y, t),
                     bil1(v0.z, v1.z, v2.z, v3.z, t), bil1(v0.w, v1.w, v2.w, v3.w, t));
}

__device__ __forceinline__ float4 sqdiff4(float4 g, float4 r) {
  const float dx = __fsub_rn(g.x, r.x), dy = __fsub_rn(g.y, r.y);
  const float dz = __fsub_rn(g.z, r.z), dw = __fsub_rn(g.w, r.w);
  return make_float4(__fmul_rn(dx, dx), __fmul_rn(dy, dy), __fmul_rn(dz, dz), __fmul_rn(dw, dw));
}

// 16-B slot s of c8 pixel p (chunk c = s >> 1, half h = s & 1) in global memory
__device__ __forceinline__ float4 ld_c8(__amdgpu_buffer_rsrc_t r, uint32_t p, int s, int HW) {
  return ld4(r, (uint32_t)(s >> 1) * (uint32_t)HW * 32u + p * 32u + 16u * (uint32_t)(s & 1));
}

// host side of cost_fwd.hip that the backward's launchers call too: the pipeline arguments
// on the workspace's c8 feature copies, and the plane strides of a group of n planes
PipeArgs pipe_args_c8(const CostArgs& ca, const SweepGeom& g, const Workspace& ws);
void group_strides(PipeArgs& a, const Workspace& ws, int n);

}  // namespace aarmvs
