// Inter-view adaptive aggregation (omega) and the per-plane cost slice for gfx950: the forward
// pipeline.  Its backward is cost_bwd.hip; the device helpers both use are in cost_device.h.
//
// Reference: models/module.py:6-38 (homo_warping_depthwise),
//            models/drmvsnet.py:27-38 (InterViewAAModule), :307-319 (accumulation).
//
// Per plane and batch element the cost slice needs three grid-wide GroupNorm
// reductions per source view.  The slices do not depend on the recurrence, so
// they are computed a plane group at a time (kPlaneGroup): one omega conv launch over the
// group's planes, two statistics launches over its 16-B/px/view omega conv output (each
// statistic reduced in a fixed order), then one cost_x launch writing the group's slices.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>

#include "cost_device.h"

namespace aarmvs {

// ---------------------------------------------------------------------------
// Cost-slice stage, per plane group d0 .. d0 + n - 1 (launch_omega_group, launch_cost_x_group):
//   omega_conv         sq_v(d) = (warp_v(d) - ref)^2 on a haloed tile in LDS, the omega
//                      conv3x3 32->4 -> t1_d (16 B/px/view), GN #0 partial sums;
//   omega_stats<1>/<2> GN #1/#2 partial sums from t1_d alone (each followed by a fixed-order
//                      stat_reduce);
//   cost_x             x_d = -(sum_v (1 + w_v) (warp_v(d) - ref)^2) / nsrc, with w_v from
//                      t1_d and plane d's three GroupNorm statistics (drmvsnet.py:307-319).
// Both gather their bilinear taps straight from the "c8" feature copies
// ([B][4][H][W][8], to_c8_kernel): one tap of one 8-channel chunk is a 32-B segment,
// and neighbouring output pixels share taps in L1/L2.
// ---------------------------------------------------------------------------
template <typename PA>
__device__ __forceinline__ void part_put(PA& a, int kp, int b, int v, int i, double s,
                                         double ss) {
  const size_t k = (((size_t)kp * a.B + b) * a.nsrc + v) * a.part_n + i;
  a.part[2 * k] = s;
  a.part[2 * k + 1] = ss;
}

__device__ __forceinline__ void gn_relu4(const float (&x)[4], const GnStat& s, const float* gw,
                                         const float* gb, bool relu, float (&y)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float sc = s.rstd * gw[c];
    const float sh = gb[c] - s.mean * sc;
    const float v = x[c] * sc + sh;
    y[c] = relu ? fmaxf(v, 0.0f) : v;
  }
}

// omega weight of one (pixel, view) from its conv3x3 output t and the three GN stats
// (drmvsnet.py:30-35 after the first conv)
__device__ __forceinline__ float omega_weight(const float4 q, const GnStat* gs, const OmegaP& o) {
  const float t[4] = {q.x, q.y, q.z, q.w};
  float aa[4], t2[4], bb[4], t3[4], g3[4];
  gn_relu4(t, gs[0], o.g0w, o.g0b, true, aa);
  conv1x1_4(aa, o.w1, o.b1, t2);
  gn_relu4(t2, gs[1], o.g1w, o.g1b, true, bb);
  conv1x1_4(bb, o.w2, o.b2, t3);
  gn_relu4(t3, gs[2], o.g2w, o.g2b, false, g3);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) s = fmaf(o.wo[c], fmaxf(g3[c] + aa[c], 0.0f), s);
  return sigmoidf_(s + o.bo);
}

// Source box of a block: the bounding box of every in-image bilinear tap its threads
// need.  Each thread extends (lx, ly, hx, hy) by its positions, then box_reduce()
// combines the block (one barrier) and returns the box in wave-uniform registers.
__device__ __forceinline__ void box_extend(const TapF& t, int H, int W, int& lx, int& ly, int& hx,
                                           int& hy) {
  if (!(t.xf == t.xf) || !(t.yf == t.yf)) return;   // NaN position: all taps read zero
  const float xl = fmaxf(t.xf, 0.f), xh = fminf(t.xf + 1.f, (float)(W - 1));
  const float yl = fmaxf(t.yf, 0.f), yh = fminf(t.yf + 1.f, (float)(H - 1));
  if (xl <= xh && yl <= yh) {
    lx = min(lx, (int)xl);
    hx = max(hx, (int)xh);
    ly = min(ly, (int)yl);
    hy = max(hy, (int)yh);
  }
}

// row of box pixel p: umulhi(p, ceil(2^32 / nx)), exact for p, nx < 2^16
// ceil(2^32 / nx) = floor((2^32 - 1) / nx) + 1: a 32-bit division (the 64-bit form cost ~110
// scalar instructions per omega item)
__device__ __forceinline__ uint32_t box_magic(int nx) {
  return nx > 1 ? 0xFFFFFFFFu / (uint32_t)nx + 1u : 0u;
}
__device__ __forceinline__ int box_row(int p, int nx, uint32_t mg) {
  return nx > 1 ? (int)__umulhi((uint32_t)p, mg) : p;
}

__device__ __forceinline__ TapP tap_p4(const TapF& t, bool valid, int H, int W, bool lds,
                                      const Box& bx, uint32_t zpix) {
  TapP o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o.wt[k] = t.wt[k];
  // tap_p's result (omega_mfma): the four taps' validity from two column and two row tests (make_taps' tests on the same
  // float coordinates), and their indices from the top-left one: one signed 24-bit multiply
  // (a tap row or column may be -1; coordinates and extents are < 2^23 wherever a tap is
  // valid, and an invalid tap's index is selected away)
  const float xf1 = t.xf + 1.0f, yf1 = t.yf + 1.0f;
  const bool cx0 = t.xf > -1.0f && t.xf < (float)W, cx1 = xf1 > -1.0f && xf1 < (float)W;
  const bool cy0 = valid && t.yf > -1.0f && t.yf < (float)H;
  const bool cy1 = valid && yf1 > -1.0f && yf1 < (float)H;
  const int ox = lds ? bx.x0 : 0, oy = lds ? bx.y0 : 0, rs = lds ? bx.nx : W;
  const int p00 = __mul24((int)t.yf - oy, rs) + ((int)t.xf - ox);
  o.pix[0] = cy0 && cx0 ? (uint32_t)p00 : zpix;
  o.pix[1] = cy0 && cx1 ? (uint32_t)(p00 + 1) : zpix;
  o.pix[2] = cy1 && cx0 ? (uint32_t)(p00 + rs) : zpix;
  o.pix[3] = cy1 && cx1 ? (uint32_t)(p00 + rs + 1) : zpix;
  return o;
}

// sample_pos split over the two lanes of a pixel: lane h computes coordinate h (x for 0,
// y for 1) with exactly sample_pos's operations, and the pair swaps results (DPP
// quad_perm [1,0,3,2]): one numerator division chain per lane instead of two.
__device__ __forceinline__ float swap_pair(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));
}
__device__ __forceinline__ void sample_pos_pair(const float* __restrict__ m, float depth, float x,
                                                float y, int H, int W, int h, float& ix,
                                                float& iy) {
  auto row = [&](int k) {
    const float rx = __fadd_rn(__fadd_rn(__fmul_rn(m[4 * k + 0], x), __fmul_rn(m[4 * k + 1], y)),
                               m[4 * k + 2]);
    return __fadd_rn(__fmul_rn(rx, depth), m[4 * k + 3]);
  };
  const float ph = h ? row(1) : row(0);
  float z = row(2);
  if (z == 0.0f) z = __fadd_rn(z, 1e-4f);
  const int dim = h ? H : W;
  const float g = __fsub_rn(__fdiv_rn(__fdiv_rn(ph, z), (float)(dim - 1) * 0.5f), 1.0f);
  const float i = __fmaf_rn(__fadd_rn(g, 1.0f), (float)dim * 0.5f, -0.5f);
  const float o = swap_pair(i);
  ix = h ? o : i;
  iy = h ? i : o;
}

// cost_x: x_d on an 8 x 32 tile, two lanes per reference pixel (lane h holds channels
// 8c + 4h .. 8c + 4h + 3 of every chunk c), so that one wave-wide tap load covers 32
// pixels x 32 B of a chunk image: contiguous 1-KiB requests.  The views are
// accumulated in view order in registers.
// XV: bit 2 (the library's) the omega weights split over the lane pair (view v by lane
// v & 1, swapped by DPP) and computed before the view loop: 0.46 vs 0.50 ms per plane;
// bit 1 (microbenchmark variant) the sampling position split over the pair as well
// (sample_pos_pair): no further gain; bits 4 / 8 (microbenchmark) 5 / 6 waves per SIMD
// instead of 4: 0.485 / 0.578 ms (6 spills) vs 0.482 ms, so occupancy is not the limit
// (the measured HBM traffic, 2.1 GB per plane, is close to the algorithmic 1.94 GB).
constexpr int kXRows = 4;   // the library's tile rows (XR): 256-thread blocks (339 vs 347 us with 8)
template <int XV = 0, int XR = kXRows>
__global__ void __launch_bounds__(2 * XR * kTileW)
__attribute__((amdgpu_waves_per_eu((XV & 8) ? 6 : (XV & 4) ? 5 : 4))) cost_x_kernel(PipeArgs a,
                                                              const float* __restrict__ P,
                                                              const float* __restrict__ Rel) {
  __shared__ GnStat gs[AARMVS_MAX_SRC][3];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int H = a.H, W = a.W, HW = H * W, nsrc = a.nsrc;
  // the npl planes of a tile are consecutive blocks of one XCD: their taps share its L2
  const int seq = xcd_tile(blockIdx.x, gridDim.x);
  const int tile = seq / a.npl, kp = seq - tile * a.npl;
  const int tiles_x = (W + kTileW - 1) / kTileW;
  const int h = tid & 1, q = tid >> 1;
  const int gy = (tile / tiles_x) * XR + q / kTileW, gx = (tile % tiles_x) * kTileW + q % kTileW;
  if (tid < 3 * nsrc) {
    const int v = tid / 3, k = tid % 3;
    gs[v][k] = stat_read(a.st_prev + kp * a.st_kstride + st_index(b, v, k, nsrc), 4.0 * HW);
  }
  __syncthreads();
  if (gy >= H || gx >= W) return;
  const float4* __restrict__ t1p = a.t1_prev + kp * a.t1_kstride;
  float* const omega_out = kp == a.omega_k ? a.omega_out : nullptr;
  // parameters come through a __restrict__ argument so that their uniform loads are
  // scalar (s_load) despite the kernel's vector stores
  OmegaP o;
  load_omega(a, P, o);
  const float dep = a.dvals[b * a.D + a.d_prev + kp];
  const uint32_t fbytes = (uint32_t)((size_t)kC * HW * 4);   // one view's c8 image
  const __amdgpu_buffer_rsrc_t rref = uniform_rsrc(a.ref + (size_t)b * kC * HW, fbytes);
  const size_t p = (size_t)gy * W + gx;
  // this lane's half of the reference feature (16 channels), read once for all views
  float4 rf[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) rf[c] = ld_c8(rref, (uint32_t)p, 2 * c + h, HW);
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  // omega weights of all views, each computed by one lane of the pair (view v by lane
  // v & 1) and swapped
  float wv[AARMVS_MAX_SRC];
#pragma unroll
  for (int vp = 0; vp < AARMVS_MAX_SRC; vp += 2) {
    if ((XV & 2) && vp < nsrc) {
      const int vm = min(vp + h, nsrc - 1);
      // 32-bit element offsets (B * nsrc * HW < 2^31, checked on the host): a wave-uniform
      // base (scalar) plus this lane's view step
      const uint32_t p32 = (uint32_t)p, hw = (uint32_t)HW;
      const float w = omega_weight(
          t1p[(uint32_t)(b * nsrc + vp) * hw + (uint32_t)(vm - vp) * hw + p32], gs[vm], o);
      if (omega_out && vp + h < nsrc)
        omega_out[(uint32_t)(vp * a.B + b) * hw + (uint32_t)(h * a.B) * hw + p32] = w;
      const float ws = swap_pair(w);
      wv[vp] = h ? ws : w;
      if (vp + 1 < AARMVS_MAX_SRC) wv[vp + 1] = h ? w : ws;
    }
  }
  for (int v = 0; v < nsrc; ++v) {
    const float* __restrict__ m = Rel + 12 * (v * a.B + b);
    const __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(a.src[v] + (size_t)b * kC * HW, fbytes);
    float w;
    if constexpr ((XV & 2) != 0) {
      w = wv[0];
#pragma unroll
      for (int k = 1; k < AARMVS_MAX_SRC; ++k) w = v == k ? wv[k] : w;
    } else {
      w = omega_weight(t1p[((size_t)b * nsrc + v) * HW + p], gs[v], o);
      if (omega_out && h == 0) omega_out[((size_t)v * a.B + b) * HW + p] = w;
    }
    const float wp1 = __fadd_rn(w, 1.0f);
    const Box none{0, 0, 0, 0};
    TapF tf;
    if constexpr ((XV & 1) == 0) {
      tf = tap_f(m, dep, gx, gy, H, W);
    } else {
      float ix, iy;
      sample_pos_pair(m, dep, (float)gx, (float)gy, H, W, h, ix, iy);
      tf.xf = floorf(ix);
      tf.yf = floorf(iy);
      const float wx = __fsub_rn(ix, tf.xf), wy = __fsub_rn(iy, tf.yf);
      const float ex = __fsub_rn(1.0f, wx), sy = __fsub_rn(1.0f, wy);
      tf.wt[0] = __fmul_rn(sy, ex);
      tf.wt[1] = __fmul_rn(sy, wx);
      tf.wt[2] = __fmul_rn(wy, ex);
      tf.wt[3] = __fmul_rn(wy, wx);
    }
    const TapP t = tap_p(tf, true, H, W, false, none, fbytes / 32u);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int s = 2 * c + h;
      const float4 g = bil4(ld_c8(rsrc, t.pix[0], s, HW), ld_c8(rsrc, t.pix[1], s, HW),
                            ld_c8(rsrc, t.pix[2], s, HW), ld_c8(rsrc, t.pix[3], s, HW), t);
      // x accumulation in view order (drmvsnet.py:311-316)
      const float4 sq = sqdiff4(g, rf[c]);
      float* ac = &acc[4 * c];
      ac[0] = __fadd_rn(ac[0], __fmul_rn(wp1, sq.x));
      ac[1] = __fadd_rn(ac[1], __fmul_rn(wp1, sq.y));
      ac[2] = __fadd_rn(ac[2], __fmul_rn(wp1, sq.z));
      ac[3] = __fadd_rn(ac[3], __fmul_rn(wp1, sq.w));
    }
  }
  // NHWC: this lane's channels 8c + 4h .. +3 of pixel p, one 16-B store per chunk
  float* xo = a.x + kp * a.x_kstride + ((size_t)b * HW + p) * kC + 4 * h;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = -1.0f * __fdiv_rn(acc[4 * c + j], (float)nsrc);
    *reinterpret_cast<float4*>(xo + 8 * c) = make_float4(r[0], r[1], r[2], r[3]);
  }
}

// cost_x with PP planes per thread: a block takes planes kp0 .. kp0 + PP - 1 of its tile (fewer
// in a ragged last block).  Consecutive planes of a sweep are spaced below a source pixel for
// most (pixel, view)s, so plane j's four taps are usually plane j - 1's.  Per view, the taps of
// the block's first plane are loaded into one register set R, and each later plane reloads R, in
// place and under a divergent branch, only in the lanes whose tap floor (xf, yf) moved (a NaN
// position never compares equal, so it reloads).  After plane j's step R holds plane j's taps in
// every lane: the taps' validity and indices follow from the floor alone, so a lane that keeps R
// reads exactly what it would have loaded.  Every (pixel, view, plane) runs cost_x_kernel<2>'s
// operations in its order: results are bit-identical for every PP (AARMVS_COST_X_PLANES).
// The omega weights (view v of a pixel computed by lane v & 1 of its pair, as there) wait in LDS,
// [plane][view][pixel], instead of PP x AARMVS_MAX_SRC registers; a pair's lanes share a wave.
template <int XR, int PP>
__global__ void __launch_bounds__(2 * XR * kTileW)
__attribute__((amdgpu_waves_per_eu(PP >= 4 ? 2 : 3))) cost_x_planes_kernel(
    PipeArgs a, const float* __restrict__ P, const float* __restrict__ Rel) {
  static_assert(3 * AARMVS_MAX_SRC * PP <= 2 * XR * kTileW, "one statistic per thread");
  __shared__ GnStat gs[PP][AARMVS_MAX_SRC][3];
  __shared__ float wl[PP][AARMVS_MAX_SRC][XR * kTileW];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int H = a.H, W = a.W, HW = H * W, nsrc = a.nsrc;
  // the plane blocks of a tile are consecutive blocks of one XCD: their taps share its L2
  const int seq = xcd_tile(blockIdx.x, gridDim.x);
  const int nkb = (a.npl + PP - 1) / PP;
  const int tile = seq / nkb, kp0 = (seq - tile * nkb) * PP;
  const int np = min(PP, a.npl - kp0);   // this block's planes
  const int tiles_x = (W + kTileW - 1) / kTileW;
  const int h = tid & 1, q = tid >> 1;
  const int gy = (tile / tiles_x) * XR + q / kTileW, gx = (tile % tiles_x) * kTileW + q % kTileW;
  if (tid < 3 * nsrc * np) {
    const int j = tid / (3 * nsrc), r = tid - j * 3 * nsrc;
    const int v = r / 3, k = r % 3;
    gs[j][v][k] =
        stat_read(a.st_prev + (kp0 + j) * a.st_kstride + st_index(b, v, k, nsrc), 4.0 * HW);
  }
  __syncthreads();
  if (gy >= H || gx >= W) return;
  const uint32_t fbytes = (uint32_t)((size_t)kC * HW * 4);   // one view's c8 image
  const size_t p = (size_t)gy * W + gx;
  float dep[PP];
  {
    OmegaP o;
    load_omega(a, P, o);
#pragma unroll
    for (int j = 0; j < PP; ++j) {
      if (j >= np) continue;
      const int kp = kp0 + j;
      dep[j] = a.dvals[b * a.D + a.d_prev + kp];
      const float4* __restrict__ t1p = a.t1_prev + kp * a.t1_kstride;
      float* const omega_out = kp == a.omega_k ? a.omega_out : nullptr;
      for (int vp = 0; vp < nsrc; vp += 2) {
        const int vm = min(vp + h, nsrc - 1);
        // 32-bit element offsets (B * nsrc * HW < 2^31, checked on the host)
        const uint32_t p32 = (uint32_t)p, hw = (uint32_t)HW;
        const float w = omega_weight(
            t1p[(uint32_t)(b * nsrc + vp) * hw + (uint32_t)(vm - vp) * hw + p32], gs[j][vm], o);
        if (vp + h < nsrc) {
          if (omega_out) omega_out[(uint32_t)(vp * a.B + b) * hw + (uint32_t)(h * a.B) * hw + p32] = w;
          wl[j][vp + h][q] = w;
        }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  // this lane's half of the reference feature (16 channels), read once for all views and planes
  const __amdgpu_buffer_rsrc_t rref = uniform_rsrc(a.ref + (size_t)b * kC * HW, fbytes);
  float4 rf[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) rf[c] = ld_c8(rref, (uint32_t)p, 2 * c + h, HW);
  float acc[PP][16];
#pragma unroll
  for (int j = 0; j < PP; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  for (int v = 0; v < nsrc; ++v) {
    const float* __restrict__ m = Rel + 12 * (v * a.B + b);
    const __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(a.src[v] + (size_t)b * kC * HW, fbytes);
    float4 R[16];   // tap k of chunk c at R[4 c + k], of the plane last stepped
    const Box none{0, 0, 0, 0};
    TapP tp[PP];
    bool moved[PP];   // plane j's tap floor differs from plane j - 1's
    float wp1[PP];
    // plane 0's loads go out first; the later planes' positions are computed under them
    {
      const TapF tf = tap_f(m, dep[0], gx, gy, H, W);
      tp[0] = tap_p(tf, true, H, W, false, none, fbytes / 32u);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) R[4 * c + k] = ld_c8(rsrc, tp[0].pix[k], 2 * c + h, HW);
      wp1[0] = __fadd_rn(wl[0][v][q], 1.0f);
      float pxf = tf.xf, pyf = tf.yf;
#pragma unroll
      for (int j = 1; j < PP; ++j) {
        if (j >= np) continue;
        const TapF tj = tap_f(m, dep[j], gx, gy, H, W);
        tp[j] = tap_p(tj, true, H, W, false, none, fbytes / 32u);
        moved[j] = !(tj.xf == pxf && tj.yf == pyf);
        pxf = tj.xf;
        pyf = tj.yf;
        wp1[j] = __fadd_rn(wl[j][v][q], 1.0f);
      }
    }
#pragma unroll
    for (int j = 0; j < PP; ++j) {
      if (j >= np) continue;
      const TapP& t = tp[j];
      // all 16 loads are issued before the first is consumed
      if (j > 0 && moved[j]) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k) R[4 * c + k] = ld_c8(rsrc, t.pix[k], 2 * c + h, HW);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 g = bil4(R[4 * c], R[4 * c + 1], R[4 * c + 2], R[4 * c + 3], t);
        // x accumulation in view order (drmvsnet.py:311-316)
        const float4 sq = sqdiff4(g, rf[c]);
        float* ac = &acc[j][4 * c];
        ac[0] = __fadd_rn(ac[0], __fmul_rn(wp1[j], sq.x));
        ac[1] = __fadd_rn(ac[1], __fmul_rn(wp1[j], sq.y));
        ac[2] = __fadd_rn(ac[2], __fmul_rn(wp1[j], sq.z));
        ac[3] = __fadd_rn(ac[3], __fmul_rn(wp1[j], sq.w));
      }
    }
  }
  // NHWC: this lane's channels 8c + 4h .. +3 of pixel p, one 16-B store per chunk and plane
#pragma unroll
  for (int j = 0; j < PP; ++j) {
    if (j >= np) continue;
    float* xo = a.x + (kp0 + j) * a.x_kstride + ((size_t)b * HW + p) * kC + 4 * h;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float r[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = -1.0f * __fdiv_rn(acc[j][4 * c + i], (float)nsrc);
      *reinterpret_cast<float4*>(xo + 8 * c) = make_float4(r[0], r[1], r[2], r[3]);
    }
  }
}

// omega_conv LDS images (source box, reference tile, sq tile): 32-B pixels (one chunk),
// the two 16-B halves of pixel p swapped when bit 3 of p is set, so that 16 consecutive
// pixels' reads of one half cover all banks.  Piece i of an image (pixel i >> 1, slot
// i & 1) sits at byte 16 i: images are lane-linear and filled by LDS-DMA.
__device__ __forceinline__ uint32_t img_slot(uint32_t p, int h) {
  return p * 8u + ((uint32_t)(h ^ (int)((p >> 3) & 1u)) << 2);
}
__device__ __forceinline__ float4 img_ld(const float* img, uint32_t p, int h) {
  return *reinterpret_cast<const float4*>(img + img_slot(p, h));
}
__device__ __forceinline__ void img_st(float* img, uint32_t p, int h, float4 v) {
  *reinterpret_cast<float4*>(img + img_slot(p, h)) = v;
}
// the half of pixel p held in slot s of its image: slot ^ swizzle bit
__device__ __forceinline__ int img_half(uint32_t p, int s) { return s ^ (int)((p >> 3) & 1u); }

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

typedef __attribute__((address_space(3))) void* lds_void_ptr;
// LDS-DMA, 16 B per lane: lane l of the wave lands at wave_dst + 16 l (wave_dst uniform);
// an offset past the buffer's range loads zeros.  soff: a wave-uniform byte offset (the chunk's
// plane) in the instruction's scalar offset, so the per-lane offset stays loop-invariant
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, float* wave_dst, uint32_t off,
                                      uint32_t soff = 0) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_ptr)wave_dst, 16, off, soff, 0, 0);
}
// hi = fp16(x) for a pair, lo = fp16(x - hi): the difference on v_fma_mix_f32 straight from
// the packed fp16 hi (x - hi is exact in fp32, so this is the same value as the convert-back
// and subtract it replaces: 4 instructions per pair instead of 6)
__device__ __forceinline__ uint32_t split_pair(float a, float b, uint32_t& lo_bits) {
  const uint32_t hb = __builtin_bit_cast(uint32_t, __builtin_convertvector((float2_t){a, b}, half2_t));
  float la, lb;
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(la) : "v"(hb), "v"(a));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(lb) : "v"(hb), "v"(b));
  lo_bits = __builtin_bit_cast(uint32_t, __builtin_convertvector((float2_t){la, lb}, half2_t));
  return hb;
}
__device__ __forceinline__ void dma_wait() {
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
}


// ---------------------------------------------------------------------------
// omega_mfma: t1 of plane d_next for one (tile, view) per block with the conv3x3 32->4 on
// the matrix cores as a GEMM followed by a shifted gather.
//
// The block owns a haloed 16 x 32 pixel tile (output: its 14 x 30 interior); wave w owns
// haloed rows 2w (lanes 0-31) and 2w+1 (lanes 32-63), one pixel per lane.  Per 8-channel
// chunk the source box arrives in LDS by LDS-DMA (as in omega_conv); each lane samples its
// own pixel (8 channels), forms sq = (warp - ref)^2 (the reference feature straight from
// the c8 image: one pixel per lane, no LDS), and splits sq 2^-e into fp16 hi + lo.  One
// v_permlane32_swap per dword pair turns the 64 lanes' (hi, lo) into the A operands of
// two v_mfma_f32_32x32x16_f16 row groups (rows = the 32 pixels of a haloed row; K =
// [8 ch hi | 8 ch lo]), and
//   Y[px][u, co] += A x [W_hi ; W_hi]  +  A x [W_lo ; 0]  +  A x [W_lo2 ; W_lo]   (u: 8 off-centre taps)
// gives hi W_hi + lo W_hi + hi W_lo + hi W_lo2 + lo W_lo (the split-fp16 product with the weights
// in three fp16 terms, DESIGN.md §Precision: no systematic per-weight error) over
// the 32 N columns (tap slot u, output channel co).  The centre tap stays an fp32 VALU
// chain on the lane's own sq.  After the 4 chunks Y goes to LDS (pixel stride 36 floats:
// conflict-free float4 reads) and each interior pixel sums its 8 neighbours' Y[., u, co].
// sq is staged x 2^-e (e from the sweep's |x| bound, ws.xbound: sq <= 4 max|feature|^2
// <= bound) so that fp16 cannot overflow; the weights carry their own power-of-two scale.
// ---------------------------------------------------------------------------
// TW: haloed tile width (32, or 16 for 256-thread blocks: 4 blocks per CU by LDS instead of 2).
// Lane l of wave w holds haloed pixel 64 w + l = (hy, hx) = ((64 w + l) / TW, (64 w + l) % TW);
// MFMA row group 0 / 1 of the wave is its lanes 0-31 / 32-63.
constexpr int kMTileH = 16;
template <int TW>
struct OmegaTile {
  static constexpr int NT = kMTileH * TW;   // threads = haloed pixels
  static constexpr int OUTH = kMTileH - 2, OUTW = TW - 2;
  static constexpr int BOXPX = 2 * NT;      // LDS source-box capacity (32-B pixels)
  static int tiles(int H, int W) { return ((W + OUTW - 1) / OUTW) * ((H + OUTH - 1) / OUTH); }
  __device__ static int tiles_d(int H, int W) { return ((W + OUTW - 1) / OUTW) * ((H + OUTH - 1) / OUTH); }
};
// the library's tile width (AARMVS_OMEGA_TW = 32: 16 x 32 haloed tiles, 512 threads; A/B builds)
#ifndef AARMVS_OMEGA_TW
#define AARMVS_OMEGA_TW 16
#endif
constexpr int kOmegaTW = AARMVS_OMEGA_TW;

// ABL: ablation bits for the diagnostic harness only (tools/microbench/pipe_bench.cpp; the
// library instantiates ABL = 0): 1 no MFMAs, 2 no box DMA, 4 no box sampling, 8 no reference
// loads, 16 sampling positions without the homography divisions (the own pixel), 32 no Y
// image / gather (t1 from the row sums of the own lanes), 64 no statistics atomics, 128 no
// fragment loads
// BAL: sign-balanced accumulation, for the training sweep only: +9% time
// wave_sum_d (device_common.h) of two values at once, in the same order and so with the same
// result, on DPP moves with an undefined `old` operand: only lane 63's value is used, and every
// lane it depends on is written at every step, so the zero fills of update_dpp are not needed
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_f64_u(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp((int)(b & 0xffffffffll), CTRL, ROWS, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, ROWS, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ void wave_sum2_d(double& u, double& w) {
  u += dpp_f64_u<0xB1, 0xF>(u);
  w += dpp_f64_u<0xB1, 0xF>(w);
  u += dpp_f64_u<0x4E, 0xF>(u);
  w += dpp_f64_u<0x4E, 0xF>(w);
  u += dpp_f64_u<0x141, 0xF>(u);
  w += dpp_f64_u<0x141, 0xF>(w);
  u += dpp_f64_u<0x140, 0xF>(u);
  w += dpp_f64_u<0x140, 0xF>(w);
  u += dpp_f64_u<0x142, 0xA>(u);
  w += dpp_f64_u<0x142, 0xA>(w);
  u += dpp_f64_u<0x143, 0xC>(u);
  w += dpp_f64_u<0x143, 0xC>(w);
  auto rl = [](double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), 63);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
  };
  u = rl(u);
  w = rl(w);
}

// one (tile, view, plane) item of omega_mfma_kernel (seq: its index in the launch's order)
// OmegaPos: the item's tile (index, row and column of tiles), source view and plane, advanced
// item by item by the kernel (no per-item integer divisions)
struct OmegaPos {
  int tile, ty, tx, v, kp;
};
// The block's GroupNorm partial of an item is summed over the block's waves one item later (by
// thread 0, after the next item's first barrier; the kernel sums the last item's after its
// loop): no barrier of its own.  wsum[par][q][wave] holds the wave sums of plane q of the item
// of parity par.
template <int NW>
__device__ __forceinline__ void omega_block_sum(const double (*ws)[2], double& s0, double& s1) {
  s0 = 0.0;
  s1 = 0.0;
  for (int w = 0; w < NW; ++w) {
    s0 += ws[w][0];
    s1 += ws[w][1];
  }
}

// LDS of an item (declared by the kernel, shared by its one- and two-plane item bodies): chunk
// c's source box and reference pixels, then (after the last chunk) the row-sum images zm, zp
// (16 B per haloed pixel each, per plane)
template <int TW>
struct OmegaLds {
  using T = OmegaTile<TW>;
  static constexpr int kRefFl = (T::BOXPX + 1) * 8;
  static constexpr int YFL = kRefFl + 2 * T::NT * 4;
  static_assert(2 * 2 * T::NT * 4 <= YFL, "two planes' row-sum images fit in the box space");
};

// PP: planes per item (1, or 2: planes ip.kp and ip.kp + 1 of one (tile, view) on one source
// box, the union of both planes' taps: one box reduce, one set of box and reference DMAs, B
// fragments and chunk barriers per pair; each plane's own arithmetic is that of PP = 1, so the
// results are bit-identical).  KPP: the kernel's largest PP (the previous item had nprev <= KPP
// planes pv.kp, pv.kp + 1, their wave sums in wsum[par ^ 1]).  PP = 2 returns false, with the
// previous item's block sums done and nothing else, when the union box does not fit the LDS
// capacity: the caller runs the two planes as single items.
template <int ABL, int TW, bool BAL, int PP, int KPP, typename PA>
__device__ __forceinline__ bool omega_item(PA& a, const float* __restrict__ P,
                                           const float* __restrict__ Rel,
                                           const unsigned* __restrict__ xbound, const OmegaPos ip,
                                           double (*wsum)[KPP][OmegaTile<TW>::NT / 64][2], int par,
                                           int nprev, const OmegaPos pv, float* const smem,
                                           int (*red)[4]) {
  using T = OmegaTile<TW>;
  constexpr int kMThreads = T::NT, kMBoxPx = T::BOXPX, kMOutH = T::OUTH, kMOutW = T::OUTW;
  constexpr int NB = (2 * kMBoxPx + kMThreads - 1) / kMThreads;   // box pieces per thread
  static_assert(TW == 16 || TW == 32, "the row sums shift by DPP along one haloed row");
  static_assert(PP == 1 || PP == 2, "one plane or a plane pair per item");
  static_assert(PP <= KPP, "the wave sums hold KPP planes per item");
  constexpr int kRefFl = OmegaLds<TW>::kRefFl;
  float* const box = smem;
  float4* const zms = reinterpret_cast<float4*>(smem);
  float4* const zps = zms + kMThreads;
  int tid;
  asm volatile("v_mov_b32 %0, %1" : "=v"(tid) : "v"((int)threadIdx.x));   // see omega_mfma_kernel
  const int lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z;
  const int H = a.H, W = a.W, HW = H * W, nsrc = a.nsrc;
  const int v = ip.v, kp = ip.kp;
  const int y0 = ip.ty * kMOutH, x0 = ip.tx * kMOutW;
  const int hy = tid / TW, hx = tid % TW;   // haloed pixel of this lane
  const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
  const bool in_img = gy >= 0 && gy < H && gx >= 0 && gx < W;
  const bool interior = in_img && hy >= 1 && hy <= kMOutH && hx >= 1 && hx <= kMOutW;
  // chunk c's reference pixels: one 16-B half per lane and DMA, half h of haloed pixel t at
  // rimg[(h NT + t) 4], after the box (conflict-free, lane-linear reads)
  float* const rimg = smem + kRefFl;

  const float* __restrict__ m = Rel + 12 * (v * a.B + b);
  const uint32_t fbytes = (uint32_t)((size_t)kC * HW * 4);
  const uint32_t cbytes = (uint32_t)HW * 32u;
  const __amdgpu_buffer_rsrc_t rref = uniform_rsrc(a.ref + (size_t)b * kC * HW, fbytes);
  const __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(a.src[v] + (size_t)b * kC * HW, fbytes);
  TapF tf[PP] = {};
  int lx = INT_MAX, ly = INT_MAX, bhx = INT_MIN, bhy = INT_MIN;
#pragma unroll
  for (int q = 0; q < PP; ++q) {
    const float dep = a.dvals[b * a.D + a.d_next + kp + q];
    if (in_img) {
      if constexpr ((ABL & 16) != 0) {
        tf[q].xf = (float)gx + 0.25f * dep * 1e-3f;
        tf[q].yf = (float)gy;
        tf[q].wt[0] = tf[q].wt[1] = tf[q].wt[2] = tf[q].wt[3] = 0.25f;
        tf[q].xf = floorf(tf[q].xf);
      } else {
        tf[q] = tap_f(m, dep, gx, gy, H, W);
      }
      box_extend(tf[q], H, W, lx, ly, bhx, bhy);
    }
  }
  const Box bx = box_reduce<kMThreads / 64>(lx, ly, bhx, bhy, red);
  // after box_reduce's barrier: every wave is past the previous item's row-sum reads and wave sums
  if constexpr (PP == 1) {
    if (tid < 8) box[kMBoxPx * 8 + tid] = 0.f;   // the zero pixel
  }
  if (nprev && tid == 0) {
#pragma unroll
    for (int q = 0; q < KPP; ++q) {
      if (q < nprev) {
        double s0, s1;
        omega_block_sum<kMThreads / 64>(wsum[par ^ 1][q], s0, s1);
        if (!(ABL & 64)) part_put(a, pv.kp + q, b, pv.v, pv.tile, s0, s1);
      }
    }
  }
  const bool lds = bx.nx * bx.ny <= min(kMBoxPx, a.box_cap);
  if constexpr (PP > 1) {
    if (!lds) return false;   // (block-uniform: bx is)
    if (tid < 8) box[kMBoxPx * 8 + tid] = 0.f;   // the zero pixel
  }
  const uint32_t zp = lds ? (uint32_t)kMBoxPx : fbytes / 32u;
  TapP tp[PP];
#pragma unroll
  for (int q = 0; q < PP; ++q) tp[q] = tap_p4(tf[q], in_img, H, W, lds, bx, zp);
  const int items = lds ? bx.nx * bx.ny * 2 : 0;
  const uint32_t mg = box_magic(bx.nx);
  uint32_t boff[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int i = tid + j * kMThreads, p = i >> 1, r = box_row(p, bx.nx, mg);
    const uint32_t gp = __umul24((uint32_t)(bx.y0 + r), (uint32_t)W) + (uint32_t)bx.x0 +
                        ((uint32_t)p - __umul24((uint32_t)r, (uint32_t)bx.nx));
    boff[j] = gp * 32u + 16u * (uint32_t)img_half((uint32_t)p, i & 1);
  }
  const uint32_t rpix = in_img ? (uint32_t)(gy * W + gx) * 32u : fbytes;
  // the wave's LDS destinations in scalar registers (m0 without a readfirstlane per DMA)
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  auto stage = [&](int c) {
    const uint32_t cb = (uint32_t)c * cbytes;
#pragma unroll
    for (int j = 0; j < NB; ++j)
      if (!(ABL & 2) && tid + j * kMThreads < items)
        dma16(rsrc, box + (j * kMThreads + wave_s * 64) * 4, boff[j], cb);
    // this lane's reference pixel in the c8 image (past the buffer: zeros)
    if (!(ABL & 8)) {
      dma16(rref, rimg + (wave_s * 64) * 4, rpix, cb);
      dma16(rref, rimg + (kMThreads + wave_s * 64) * 4, rpix + 16u, cb);
    }
  };
  // sq staging scale: bound 2^-e in [2^13, 2^15) (sq <= 4 max|f|^2 <= bound), e even and of
  // either sign, so that fp16 cannot overflow and the lo parts of small sq stay normal numbers.
  // The scale is applied as 2^(-e/2) to the difference: the bilinear weights carry it (the
  // sample is 2^(-e/2) g exactly) and the reference is subtracted by one fma with -2^(-e/2),
  // so sq arrives scaled with no multiply of its own; the centre tap accumulates the scaled sq
  // and is scaled back by 2^e at the end (all exact power-of-two scalings)
  int e = 0;
  {
    const float bound = __uint_as_float(*xbound);
    if (bound > 0.0f) {
      const int k = ilogbf(bound);
      e = k >= 134 ? 120 : (k < -100 ? -114 : k - 14);
      e += e & 1;
    }
  }
  const float dsc = ldexpf(1.0f, -(e / 2));
#pragma unroll
  for (int q = 0; q < PP; ++q)
#pragma unroll
    for (int k = 0; k < 4; ++k) tp[q].wt[k] = __fmul_rn(tp[q].wt[k], dsc);
  const float* __restrict__ w0t = P + a.off_ow0t;   // [9][32][4]: centre tap = tap 4
  const half8* __restrict__ owm = reinterpret_cast<const half8*>(P + a.off_owm);
  floatx16 acc0[PP], acc1[PP];   // first written by chunk 0's MFMAs (ABL 1: zero here)
  if constexpr ((ABL & 1) != 0) {
#pragma unroll
    for (int q = 0; q < PP; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[q][r] = acc1[q][r] = 0.f;
  }
  float o4[PP][4] = {};

  stage(0);
  dma_wait();
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < 4; ++c) {
    const float* const bx_c = box;
    // the reference pixel from LDS (DMA'd with the box: a register prefetch carried across
    // the chunk loop cost 16 register copies per chunk)
    // (a pair reads it once, ahead of both planes' sampling; one plane after its box reads)
    float4 rf0, rf1;
    auto ref_read = [&]() {
      rf0 = *reinterpret_cast<const float4*>(rimg + tid * 4);
      rf1 = *reinterpret_cast<const float4*>(rimg + (kMThreads + tid) * 4);
    };
    if constexpr (PP > 1) ref_read();
    // sq 2^-e: (2^(-e/2) g - 2^(-e/2) r)^2, the difference rounded once as in sqdiff4
    auto dsq = [&](float g, float r) {
      const float dd = __fmaf_rn(r, -dsc, g);
      return __fmul_rn(dd, dd);
    };
    // sample the own pixel (8 channels) of plane q and form sq
    auto sample = [&](int q, float (&sq)[8]) {
      const TapP& t = tp[q];
      float4 g0, g1;
      if (ABL & 4) {
        g0 = g1 = make_float4(t.wt[0], t.wt[1], t.wt[2], t.wt[3]);
      } else if (PP > 1 || lds) {
        g0 = bil4(img_ld(bx_c, t.pix[0], 0), img_ld(bx_c, t.pix[1], 0), img_ld(bx_c, t.pix[2], 0),
                  img_ld(bx_c, t.pix[3], 0), t);
        g1 = bil4(img_ld(bx_c, t.pix[0], 1), img_ld(bx_c, t.pix[1], 1), img_ld(bx_c, t.pix[2], 1),
                  img_ld(bx_c, t.pix[3], 1), t);
      } else {
        g0 = bil4(ld_c8(rsrc, t.pix[0], 2 * c, HW), ld_c8(rsrc, t.pix[1], 2 * c, HW),
                  ld_c8(rsrc, t.pix[2], 2 * c, HW), ld_c8(rsrc, t.pix[3], 2 * c, HW), t);
        g1 = bil4(ld_c8(rsrc, t.pix[0], 2 * c + 1, HW), ld_c8(rsrc, t.pix[1], 2 * c + 1, HW),
                  ld_c8(rsrc, t.pix[2], 2 * c + 1, HW), ld_c8(rsrc, t.pix[3], 2 * c + 1, HW), t);
      }
      if constexpr (PP == 1) ref_read();
      sq[0] = dsq(g0.x, rf0.x);
      sq[1] = dsq(g0.y, rf0.y);
      sq[2] = dsq(g0.z, rf0.z);
      sq[3] = dsq(g0.w, rf0.w);
      sq[4] = dsq(g1.x, rf1.x);
      sq[5] = dsq(g1.y, rf1.y);
      sq[6] = dsq(g1.z, rf1.z);
      sq[7] = dsq(g1.w, rf1.w);
    };
    half8 Bd, Bl, Bl2;
    // plane q's centre tap, fp16 split and MFMAs on its sq
    auto accumulate = [&](int q, const float (&sq)[8]) {
      // centre tap (omega.reweight_network.0.0, tap 4) on the own pixel, fp32 (BAL)
      {
        const float* wt = w0t + (4 * kC + 8 * c) * 4;
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int co = 0; co < 4; ++co) o4[q][co] = fmaf(sq[j], wt[j * 4 + co], o4[q][co]);
      }
      // split sq 2^-e into fp16 hi + lo.  Out-of-image pixels (the conv's zero padding) already
      // have sq = 0: zero bilinear weights on the box's zero pixel (or past the buffer) and a
      // reference read past the buffer.  Two values per v_cvt_pk_f16_f32.
      uint32_t hw[4], lw[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) hw[i] = split_pair(sq[2 * i], sq[2 * i + 1], lw[i]);
      // after the swaps, (hw, lw) are the pixel operands of the wave's pixels 0-31 (lanes 0-31
      // hi, 32-63 lo of pixel lane & 31) and of its pixels 32-63
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const auto r = __builtin_amdgcn_permlane32_swap(hw[i], lw[i], false, false);
        hw[i] = r[0];
        lw[i] = r[1];
      }
      // BAL: odd chunks accumulate the negated sum (accumulators and A negated), so the matrix
      // cores' downward rounding alternates sign
      if (BAL && (c & 1)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          hw[i] ^= 0x80008000u;
          lw[i] ^= 0x80008000u;
        }
      }
      if (BAL && c > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc0[q][r] = -acc0[q][r];
          acc1[q][r] = -acc1[q][r];
        }
      }
      const half8 A0 = __builtin_bit_cast(half8, u32x4{hw[0], hw[1], hw[2], hw[3]});
      const half8 A1 = __builtin_bit_cast(half8, u32x4{lw[0], lw[1], lw[2], lw[3]});
      if constexpr ((ABL & 128) != 0) {
        Bd = A1;
        Bl = A0;
        Bl2 = A1;
      }
      // D^T = W x [sq hi | sq lo]^T: the weight fragments as the A operand, so that a lane holds
      // its pixel's tap slots (rows) rather than a slot's pixels: row r of lane l is slot
      // 2 (r >> 2) + (l >> 5), output channel r & 3 (the row sums below)
      if (!(ABL & 1)) {
        if (c == 0) {   // the accumulators start from the MFMA's inline-zero C operand (no zero fill)
          const floatx16 z = {};
          acc0[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bd, A0, z, 0, 0, 0);
          acc1[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bd, A1, z, 0, 0, 0);
        } else {
          acc0[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bd, A0, acc0[q], 0, 0, 0);
          acc1[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bd, A1, acc1[q], 0, 0, 0);
        }
        acc0[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bl, A0, acc0[q], 0, 0, 0);
        acc1[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bl, A1, acc1[q], 0, 0, 0);
        acc0[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bl2, A0, acc0[q], 0, 0, 0);
        acc1[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bl2, A1, acc1[q], 0, 0, 0);
      } else {
        acc0[q][0] += (float)A0[0] + (float)Bd[1];
        acc1[q][0] += (float)A1[0] + (float)Bl[1];
      }
    };
    // this chunk's B fragments, issued before the barrier: their L1/L2 latency is hidden
    // behind it and the centre-tap chain (2.5% of the kernel against loading them after;
    // DMA'ing all 12 to LDS once per item instead was 1.8%)
    auto fragments = [&]() {
      if constexpr ((ABL & 128) == 0) {
        Bd = owm[(c * 3 + 0) * 64 + lane];
        Bl = owm[(c * 3 + 1) * 64 + lane];
        Bl2 = owm[(c * 3 + 2) * 64 + lane];
      }
    };
    // Every plane samples first: the barrier then frees the box for chunk c + 1's DMA, which
    // runs under all the planes' arithmetic.  (A pair that accumulated its first plane before
    // sampling the second held the reference pixel and the fragments across that sampling:
    // 168 VGPRs with 11 spilled; this order holds 8 sq values instead.)
    float sq[PP][8];
#pragma unroll
    for (int q = 0; q < PP; ++q) {
      // (one plane's eight box reads at a time: all sixteen in flight spilled 52 VGPRs)
      sample(q, sq[q]);
      // a pair's sq are formed here, plane by plane: left to itself the compiler keeps both
      // planes' sixteen box reads in flight and sinks the bilinear chains below the barrier
      // (64 VGPRs of taps across it: 52 spilled)
      if constexpr (PP > 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(sq[q][j]));
      }
    }
    fragments();
    __syncthreads();   // every lane's box and reference reads of chunk c are done
    if (c < 3) stage(c + 1);
#pragma unroll
    for (int q = 0; q < PP; ++q) accumulate(q, sq[q]);
    if (c < 3) {
      dma_wait();
      __syncthreads();   // chunk c+1's box and reference visible
    }
  }
  // The 3x3 conv's off-centre taps as row sums, in registers.  acc0 / acc1 hold the wave's
  // pixels 0-31 / 32-63 (pixel lane & 31 in lanes l and l + 32); register group g (registers
  // 4 g .. 4 g + 3, output channels 0-3) holds tap slot 2 g in lanes 0-31 and 2 g + 1 in lanes
  // 32-63, slots -> taps 0, 6 | 1, 7 | 2, 8 | 3, 5 (pack_omega_conv_kernel): the groups 0-2 are
  // the taps of dx = -1, 0, +1 of row dy = -1 (lanes 0-31) and dy = +1 (lanes 32-63).  A 16-lane
  // DPP row is one haloed row (TW = 16), so the dx neighbours are one lane away:
  //   Z_dy[q] = Y(dy,-1)[q - 1] + Y(dy,0)[q] + Y(dy,+1)[q + 1]          (row_shr / row_shl)
  //   Z_0[q]  = Y(0,-1)[q - 1] + Y(0,+1)[q + 1]
  //   t1[p]   = Z_-1[p - TW] + Z_0[p] + Z_+1[p + TW]                    (via LDS: other waves)
  // (the edge lanes of a row get zeros from the DPP bound: they are halo pixels, never output).
  // TW = 32: a haloed row is a lane half, two DPP rows; wave_shr / wave_shl shift across them,
  // and the lanes a shift carries across a half or the wave's end are halo columns too.
  static constexpr int kShr = TW == 16 ? 0x111 : 0x138, kShl = TW == 16 ? 0x101 : 0x130;
  auto shr1 = [](float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), kShr, 0xF, 0xF, true));
  };
  auto shl1 = [](float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), kShl, 0xF, 0xF, true));
  };
  // (plane q's images at zms / zps + 2 q NT)
  float zmr[PP][4], zpr[PP][4], z0[PP][4];
#pragma unroll
  for (int q = 0; q < PP; ++q) {
#pragma unroll
    for (int co = 0; co < 4; ++co) {
      const float r0 = (shr1(acc0[q][co]) + acc0[q][4 + co]) + shl1(acc0[q][8 + co]);
      const float r1 = (shr1(acc1[q][co]) + acc1[q][4 + co]) + shl1(acc1[q][8 + co]);
      // -> Z_-1 of the wave's pixel `lane` in zmr, Z_+1 in zpr
      const auto zz = __builtin_amdgcn_permlane32_swap(__float_as_uint(r0), __float_as_uint(r1), false, false);
      zmr[q][co] = __uint_as_float(zz[0]);
      zpr[q][co] = __uint_as_float(zz[1]);
      // -> tap 3 and tap 5 of pixel `lane`
      const auto t35 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc0[q][12 + co]),
                                                        __float_as_uint(acc1[q][12 + co]), false, false);
      z0[q][co] = shr1(__uint_as_float(t35[0])) + shl1(__uint_as_float(t35[1]));
    }
    // the row-sum images over the box space: every lane passed chunk 3's box reads before the
    // barrier in the loop
    if constexpr ((ABL & 32) == 0) {
      zms[2 * q * kMThreads + tid] = make_float4(zmr[q][0], zmr[q][1], zmr[q][2], zmr[q][3]);
      zps[2 * q * kMThreads + tid] = make_float4(zpr[q][0], zpr[q][1], zpr[q][2], zpr[q][3]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PP; ++q) {
    // GroupNorm partials in fp64 from the first addition on (var = E[x^2] - E[x]^2 cancels)
    double ps = 0.0, pss = 0.0;
    if (interior) {
      float g4[4];
      if constexpr ((ABL & 32) != 0) {
#pragma unroll
        for (int co = 0; co < 4; ++co) g4[co] = (zmr[q][co] + z0[q][co]) + zpr[q][co];
      } else {
        const float4 up = zms[2 * q * kMThreads + tid - TW], dn = zps[2 * q * kMThreads + tid + TW];
        g4[0] = (up.x + z0[q][0]) + dn.x;
        g4[1] = (up.y + z0[q][1]) + dn.y;
        g4[2] = (up.z + z0[q][2]) + dn.z;
        g4[3] = (up.w + z0[q][3]) + dn.w;
      }
      if (BAL) {   // chunk 3 left -sum in the accumulators
#pragma unroll
        for (int co = 0; co < 4; ++co) g4[co] = -g4[co];
      }
      const float pe = ldexpf(1.0f, e);
      const float isc = P[a.off_owm_scale] * pe;
      const float* __restrict__ b0 = P + a.off_ob0;
      float4 out;
      out.x = fmaf(g4[0], isc, o4[q][0] * pe) + b0[0];
      out.y = fmaf(g4[1], isc, o4[q][1] * pe) + b0[1];
      out.z = fmaf(g4[2], isc, o4[q][2] * pe) + b0[2];
      out.w = fmaf(g4[3], isc, o4[q][3] * pe) + b0[3];
      a.t1_next[(kp + q) * a.t1_kstride + ((size_t)b * nsrc + v) * HW + gy * W + gx] = out;
      ps = ((double)out.x + (double)out.y) + ((double)out.z + (double)out.w);
      pss = ((double)out.x * out.x + (double)out.y * out.y) + ((double)out.z * out.z + (double)out.w * out.w);
    }
    wave_sum2_d(ps, pss);
    if (lane == 0) {
      wsum[par][q][wave][0] = ps;
      wsum[par][q][wave][1] = pss;
    }
  }
  return true;
}

// The kernel: a block takes a.omega_ipb consecutive items (omega_ipb()).  A tile's (view, plane)
// items are consecutive on one XCD (xcd_tile): the reference tile, and a view's source box
// across the npl neighbouring planes, come from its L2.
// (AARMVS_OMEGA_WAVES: the minimum waves per SIMD the compiler is held to; A/B builds only)
#ifndef AARMVS_OMEGA_WAVES
#define AARMVS_OMEGA_WAVES 4
#endif
// KPP = 2: items seq, seq + 1 of a block that are planes kp, kp + 1 of one (tile, view) run as
// one plane-pair item (omega_item's PP = 2); a last odd item, or a pair whose union box does not
// fit the LDS capacity, runs as today's single items.  The pair's second accumulators cost a
// wave per SIMD (3).  Grid, tile order and the meaning of omega_ipb (planes per block) do not
// depend on KPP.  KPP = 1 keeps the one-plane kernel's item loop as it was.
template <int ABL = 0, int TW = kOmegaTW, bool BAL = false, int KPP = 1>
__global__ void __launch_bounds__(OmegaTile<TW>::NT)
__attribute__((amdgpu_waves_per_eu(KPP > 1 ? 3 : AARMVS_OMEGA_WAVES)))
omega_mfma_kernel(PipeArgs a, const float* __restrict__ P, const float* __restrict__ Rel,
                  const unsigned* __restrict__ xbound) {
  if (blockDim.x != OmegaTile<TW>::NT) return;   // LDS images are sized for exactly this block
  __shared__ __attribute__((aligned(16))) float smem[OmegaLds<TW>::YFL];
  // box_reduce's scratch: the pair attempt has its own, since a pair that does not fit is
  // followed by a single item's reduce with no barrier between
  __shared__ int red[KPP][OmegaTile<TW>::NT / 64][4];
  const int ipb = a.omega_ipb > 1 ? a.omega_ipb : 1;
  const int npl = a.npl, nsrc = a.nsrc;
  const int tiles_x = (a.W + OmegaTile<TW>::OUTW - 1) / OmegaTile<TW>::OUTW;
  const int total = OmegaTile<TW>::tiles_d(a.H, a.W) * nsrc * npl;
  const int seq0 = xcd_tile(blockIdx.x, gridDim.x) * ipb;
  // seq = (tile * nsrc + v) * npl + kp, decomposed once and then advanced
  OmegaPos ip;
  ip.tile = seq0 / (nsrc * npl);
  {
    const int vk = seq0 - ip.tile * (nsrc * npl);
    ip.v = vk / npl;
    ip.kp = vk - ip.v * npl;
    ip.ty = ip.tile / tiles_x;
    ip.tx = ip.tile - ip.ty * tiles_x;
  }
  constexpr int NW = OmegaTile<TW>::NT / 64;
  __shared__ double wsum[2][KPP][NW][2];
  OmegaPos pv = ip;
  if constexpr (KPP == 1) {
    int it = 0;
#pragma unroll 1
    for (; it < ipb; ++it) {
      if (seq0 + it >= total) break;
      // (no barrier between items: the next item's LDS writes all follow box_reduce's barrier,
      // which every wave reaches after the previous item's last LDS read)
      if (it) {
        pv = ip;
        if (++ip.kp == npl) {
          ip.kp = 0;
          if (++ip.v == nsrc) {
            ip.v = 0;
            ++ip.tile;
            if (++ip.tx == tiles_x) {
              ip.tx = 0;
              ++ip.ty;
            }
          }
        }
      }
      // the item reads the arguments through a pointer the compiler cannot prove invariant
      // across items: otherwise it hoists every argument load out of the loop (SGPR spills)
      uint32_t z;
      asm volatile("s_mov_b32 %0, 0" : "=s"(z));
      typedef const __attribute__((address_space(4))) PipeArgs KPipeArgs;
      KPipeArgs& ka = *(KPipeArgs*)((const __attribute__((address_space(4))) char*)&a + z);
      omega_item<ABL, TW, BAL, 1, 1>(ka, P, Rel, xbound, ip, wsum, it & 1, it > 0, pv, smem, red[0]);
    }
    if (it > 0) {   // the last item's block sum
      __syncthreads();
      if (threadIdx.x == 0) {
        double s0, s1;
        omega_block_sum<NW>(wsum[(it - 1) & 1][0], s0, s1);
        if (!(ABL & 64)) part_put(a, ip.kp, (int)blockIdx.z, ip.v, ip.tile, s0, s1);
      }
    }
  } else {
    // it: planes done; np: planes of the item that ran last (0: none, or its block sums are done);
    // par: parity of the items run; singles: planes left of a pair that runs as single items
    int it = 0, np = 0, par = 0, singles = 0;
#pragma unroll 1
    while (it < ipb && seq0 + it < total) {
      // (no barrier between items: the next item's LDS writes all follow box_reduce's barrier,
      // which every wave reaches after the previous item's last LDS read)
      // the item reads the arguments through a pointer the compiler cannot prove invariant
      // across items: otherwise it hoists every argument load out of the loop (SGPR spills)
      uint32_t z;
      asm volatile("s_mov_b32 %0, 0" : "=s"(z));
      typedef const __attribute__((address_space(4))) PipeArgs KPipeArgs;
      KPipeArgs& ka = *(KPipeArgs*)((const __attribute__((address_space(4))) char*)&a + z);
      int done = 0;
      if (singles == 0 && it + 1 < ipb && seq0 + it + 1 < total && ip.kp + 1 < npl) {
        if (omega_item<ABL, TW, BAL, 2, KPP>(ka, P, Rel, xbound, ip, wsum, par, np, pv, smem, red[1]))
          done = 2;
        else {
          np = 0;
          singles = 2;
        }
      }
      if (done == 0) {
        omega_item<ABL, TW, BAL, 1, KPP>(ka, P, Rel, xbound, ip, wsum, par, np, pv, smem, red[0]);
        done = 1;
        if (singles) --singles;
      }
      pv = ip;
      np = done;
      par ^= 1;
      it += done;
      ip.kp += done;
      if (ip.kp == npl) {   // (a pair never crosses a view's last plane)
        ip.kp = 0;
        if (++ip.v == nsrc) {
          ip.v = 0;
          ++ip.tile;
          if (++ip.tx == tiles_x) {
            ip.tx = 0;
            ++ip.ty;
          }
        }
      }
    }
    if (np > 0) {   // the last item's block sums
      __syncthreads();
      if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < KPP; ++q) {
          if (q < np) {
            double s0, s1;
            omega_block_sum<NW>(wsum[par ^ 1][q], s0, s1);
            if (!(ABL & 64)) part_put(a, pv.kp + q, (int)blockIdx.z, pv.v, pv.tile, s0, s1);
          }
        }
      }
    }
  }
}

// GN #STAGE (1 or 2) partial sums of the omega chain on t1 (plane d_next).
template <int STAGE>
__global__ void __launch_bounds__(256) omega_stats_kernel(PipeArgs a,
                                                          const float* __restrict__ P) {
  __shared__ double red[2 * 4];
  __shared__ GnStat gs[2];
  const int v = blockIdx.y, b = blockIdx.z / a.npl, kp = blockIdx.z - b * a.npl;
  const int HW = a.H * a.W;
  double* const st = a.st_next + kp * a.st_kstride;
  if (threadIdx.x < STAGE)
    gs[threadIdx.x] = stat_read(st + st_index(b, v, threadIdx.x, a.nsrc), 4.0 * HW);
  __syncthreads();
  OmegaP o;
  load_omega(a, P, o);
  const float4* t1 = a.t1_next + kp * a.t1_kstride + ((size_t)b * a.nsrc + v) * HW;
  double part[2] = {0.0, 0.0};   // fp64: var = E[x^2] - E[x]^2 cancels
  // four independent 16-B loads in flight per thread per iteration
  const int gstride = gridDim.x * blockDim.x;
  for (int p0 = blockIdx.x * blockDim.x + threadIdx.x; p0 < HW; p0 += 4 * gstride) {
    float4 qs[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = p0 + u * gstride;
      qs[u] = p < HW ? t1[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
    if (p0 + u * gstride >= HW) break;
    const float4 q = qs[u];
    const float t[4] = {q.x, q.y, q.z, q.w};
    float aa[4], t2[4];
    gn_relu4(t, gs[0], o.g0w, o.g0b, true, aa);
    conv1x1_4(aa, o.w1, o.b1, t2);
    float r[4];
    if constexpr (STAGE == 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) r[c] = t2[c];
    } else {
      float bb[4];
      gn_relu4(t2, gs[1], o.g1w, o.g1b, true, bb);
      conv1x1_4(bb, o.w2, o.b2, r);
    }
    part[0] += ((double)r[0] + (double)r[1]) + ((double)r[2] + (double)r[3]);
    part[1] += ((double)r[0] * r[0] + (double)r[1] * r[1]) + ((double)r[2] * r[2] + (double)r[3] * r[3]);
    }
  }
  block_sum_d<2>(part, red);
  if (threadIdx.x == 0) part_put(a, kp, b, v, blockIdx.x, part[0], part[1]);
}

// Statistic STAGE of every (plane, batch element, view) of a group from the per-block
// partials: one block per (plane, b, v), each thread a strided sequential sum, then a fixed
// tree; the result goes to slot 0 of the statistic (the other slots stay zero).
__global__ void __launch_bounds__(256) stat_reduce_kernel(PipeArgs a, int stage) {
  __shared__ double red[2][256];
  const int g = blockIdx.x, v = g % a.nsrc, b = (g / a.nsrc) % a.B, kp = g / (a.nsrc * a.B);
  const double* pp = a.part + 2 * (size_t)g * a.part_n;
  double s = 0.0, ss = 0.0;
  for (int i = threadIdx.x; i < a.part_n; i += 256) {
    s += pp[2 * i];
    ss += pp[2 * i + 1];
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = ss;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* st = a.st_next + kp * a.st_kstride + st_index(b, v, stage, a.nsrc);
    st[0] = red[0][0];
    st[1] = red[1][0];
  }
}

static PipeArgs pipe_args(const CostArgs& ca, const SweepGeom& g, const Workspace& ws) {
  const ParamLayout& L = param_layout();
  PipeArgs a{};
  a.ref = ca.ref;
  for (int v = 0; v < AARMVS_MAX_SRC; ++v) a.src[v] = v < g.nsrc ? ca.src[v] : nullptr;
  a.rel = ca.rel;
  a.dvals = ca.depth_values;
  a.D = g.D;
  a.params = ca.params;
  a.x = ws.x;
  a.B = g.B;
  a.H = g.H;
  a.W = g.W;
  a.nsrc = g.nsrc;
  a.box_cap = INT_MAX;
  a.npl = 1;
  a.omega_k = 0;
  a.off_ow0 = L.pk_off[P_OW0];
  a.off_ow0t = L.ow0t_off;
  a.off_owb_scale = L.owb_scale_off;
  a.off_owm = L.owm_off;
  a.off_owm_scale = L.owb_scale_off;
  a.off_ob0 = L.pk_off[P_OB0];
  a.off_og0w = L.pk_off[P_OG0W];
  a.off_og0b = L.pk_off[P_OG0B];
  a.off_ow1 = L.pk_off[P_OW1];
  a.off_ob1 = L.pk_off[P_OB1];
  a.off_og1w = L.pk_off[P_OG1W];
  a.off_og1b = L.pk_off[P_OG1B];
  a.off_ow2 = L.pk_off[P_OW2];
  a.off_ob2 = L.pk_off[P_OB2];
  a.off_og2w = L.pk_off[P_OG2W];
  a.off_og2b = L.pk_off[P_OG2B];
  a.off_owo = L.pk_off[P_OWO];
  a.off_obo = L.pk_off[P_OBO];
  return a;
}

// LDS source-box capacity override: AARMVS_PIPE_BOX_CAP=n (pixels) forces smaller boxes,
// i.e. cost_x's region subdivision and omega_conv's global-gather fallback (a diagnostic
// for the parity tests; results are bit-identical)
static int pipe_box_cap() {
  const char* s = std::getenv("AARMVS_PIPE_BOX_CAP");
  return (s && *s) ? std::max(4, std::atoi(s)) : INT_MAX;
}

// omega_mfma items per block: a block walks ipb consecutive (plane) items of one (tile, view),
// so its fixed cost (prologue, box set-up, statistics hand-off) is paid once per ipb items:
// -3..10% omega time at the headline geometry.  Default 4, halved while the
// grid would hold fewer than 8 blocks per CU; AARMVS_OMEGA_IPB=n forces n (results are
// bit-identical for every n: the items' arithmetic does not change).
static int omega_ipb(int items, int cu_count) {
  const char* s = std::getenv("AARMVS_OMEGA_IPB");
  if (s && *s) return std::max(1, std::min(8, std::atoi(s)));
  // 8 items per block where the grid stays >= 8 blocks per CU (round 6, second session: 7.58-7.61
  // against 7.65-7.67 ms per headline launch at 4, profiles/r06s14_omega_ipb.txt)
  int ipb = 8;
  while (ipb > 1 && (items + ipb - 1) / ipb < 8 * std::max(1, cu_count)) ipb >>= 1;
  return ipb;
}

// omega_mfma planes per item of the inference sweep (omega_mfma_kernel's KPP):
// AARMVS_OMEGA_PLANES=1|2, read per launch, for A/B runs and the tests (results are
// bit-identical for both values).  Default 2: the measurements are in DESIGN.md section 4 and
// profiles/omega_planes_ab.txt.
constexpr int kOmegaPlanes = 2;
static int omega_planes() {
  const char* s = std::getenv("AARMVS_OMEGA_PLANES");
  const int v = (s && *s) ? std::atoi(s) : kOmegaPlanes;
  return v >= 2 ? 2 : 1;
}

// cost_x planes per thread (cost_x_kernel's PP): AARMVS_COST_X_PLANES=1|2|4 forces it for A/B
// runs and the tests (results are bit-identical for every value)
constexpr int kCostXPlanes = 2;
static int cost_x_planes() {
  const char* s = std::getenv("AARMVS_COST_X_PLANES");
  const int v = (s && *s) ? std::atoi(s) : kCostXPlanes;
  return v >= 4 ? 4 : v >= 2 ? 2 : 1;
}

PipeArgs pipe_args_c8(const CostArgs& ca, const SweepGeom& g, const Workspace& ws) {
  PipeArgs a = pipe_args(ca, g, ws);
  // the pipeline reads the c8 copies of the features in the workspace
  a.ref = ws.feat8[0];
  for (int v = 0; v < g.nsrc; ++v) a.src[v] = ws.feat8[1 + v];
  a.box_cap = pipe_box_cap();
  return a;
}

void group_strides(PipeArgs& a, const Workspace& ws, int n) {
  a.npl = n;
  a.t1_kstride = ws.t1_plane;
  a.st_kstride = ws.omega_stats_bytes / sizeof(double);
  a.x_kstride = ws.x_plane;
}

hipError_t launch_cost_x_group(const CostArgs& ca, const SweepGeom& g, const Workspace& ws, int d0,
                               int n, float* x0, float* omega_out, int omega_k, hipStream_t s) {
  PipeArgs a = pipe_args_c8(ca, g, ws);
  group_strides(a, ws, n);
  a.d_prev = d0;
  a.d_next = -1;
  a.x = x0;
  a.t1_prev = reinterpret_cast<const float4*>(ws.t1);
  a.st_prev = ws.omega_stats;
  a.omega_out = omega_out;
  a.omega_k = omega_out ? omega_k : -1;
  const int ntiles = ((g.W + kTileW - 1) / kTileW) * ((g.H + kXRows - 1) / kXRows);
  const int pp = cost_x_planes();
  const dim3 grid(ntiles * ((n + pp - 1) / pp), g.B), block(2 * kXRows * kTileW);
  ProfScope ps(s, K_COST_X);
  if (pp == 4)
    hipLaunchKernelGGL((cost_x_planes_kernel<kXRows, 4>), grid, block, 0, s, a, a.params, a.rel);
  else if (pp == 2)
    hipLaunchKernelGGL((cost_x_planes_kernel<kXRows, 2>), grid, block, 0, s, a, a.params, a.rel);
  else
    hipLaunchKernelGGL(cost_x_kernel<2>, grid, block, 0, s, a, a.params, a.rel);
  return hipGetLastError();
}

hipError_t launch_omega_group(const CostArgs& ca, const SweepGeom& g, const Workspace& ws, int d0,
                              int n, hipStream_t s, bool balanced) {
  PipeArgs a = pipe_args_c8(ca, g, ws);
  group_strides(a, ws, n);
  a.d_prev = -1;
  a.d_next = d0;
  a.t1_next = reinterpret_cast<float4*>(ws.t1);
  a.st_next = ws.omega_stats;
  a.part = ws.omega_part;
  hipError_t e;
  const int nred = n * g.B * g.nsrc;   // reduce blocks
  // the group's statistics accumulate from zero
  if ((e = hipMemsetAsync(ws.omega_stats, 0, (size_t)n * ws.omega_stats_bytes, s)) != hipSuccess)
    return e;
  {
    const int ntiles = OmegaTile<kOmegaTW>::tiles(g.H, g.W);
    ProfScope ps(s, K_OMEGA_CONV);
    a.part_n = ntiles;
    a.omega_ipb = omega_ipb(ntiles * g.nsrc * n * g.B, g.cu_count);
    const int nblk = (ntiles * g.nsrc * n + a.omega_ipb - 1) / a.omega_ipb;
    if (balanced)   // (the training sweep stays at one plane per item)
      hipLaunchKernelGGL((omega_mfma_kernel<0, kOmegaTW, true>), dim3(nblk, 1, g.B),
                         dim3(OmegaTile<kOmegaTW>::NT), 0, s, a, a.params, a.rel, ws.xbound);
    else if (n > 1 && a.omega_ipb > 1 && omega_planes() == 2)
      hipLaunchKernelGGL((omega_mfma_kernel<0, kOmegaTW, false, 2>), dim3(nblk, 1, g.B),
                         dim3(OmegaTile<kOmegaTW>::NT), 0, s, a, a.params, a.rel, ws.xbound);
    else
      hipLaunchKernelGGL((omega_mfma_kernel<0, kOmegaTW>), dim3(nblk, 1, g.B),
                         dim3(OmegaTile<kOmegaTW>::NT), 0, s, a, a.params, a.rel, ws.xbound);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  {
    ProfScope ps(s, K_STAT_REDUCE);
    hipLaunchKernelGGL(stat_reduce_kernel, dim3(nred), dim3(256), 0, s, a, 0);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // GN #1 / #2 statistics of every plane of the group.  The blocks per (plane, view) must
  // not depend on n: the fp32 per-thread partial sums follow the grid stride, and a plane's
  // statistics are bit-identical however the sweep is grouped or split into d_range calls.
  const int HW = g.H * g.W;
  const int pblk =
      std::max(1, std::min((HW + 1023) / 1024, 8 * g.cu_count / std::max(1, g.B * g.nsrc) + 1));
  a.part_n = pblk;
  {
    ProfScope ps(s, K_OMEGA1);
    hipLaunchKernelGGL(omega_stats_kernel<1>, dim3(pblk, g.nsrc, g.B * n), dim3(256), 0, s, a,
                       a.params);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  {
    ProfScope ps(s, K_STAT_REDUCE);
    hipLaunchKernelGGL(stat_reduce_kernel, dim3(nred), dim3(256), 0, s, a, 1);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  {
    ProfScope ps(s, K_OMEGA2);
    hipLaunchKernelGGL(omega_stats_kernel<2>, dim3(pblk, g.nsrc, g.B * n), dim3(256), 0, s, a,
                       a.params);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  {
    ProfScope ps(s, K_STAT_REDUCE);
    hipLaunchKernelGGL(stat_reduce_kernel, dim3(nred), dim3(256), 0, s, a, 2);
  }
  return hipGetLastError();
}

// NCHW [B][32][HW] -> c8 [B][4][HW][8] (once per sweep): four 8-channel chunk images of
// 32-B pixels.  64 pixels per block through LDS: coalesced reads and 16-B writes.
__global__ void __launch_bounds__(256) nchw_to_c8_kernel(const float* __restrict__ src,
                                                         float* __restrict__ dst, int HW,
                                                         unsigned* __restrict__ xbound) {
  __shared__ float t[kC][65];
  __shared__ float wmax[4];
  const int b = blockIdx.y, p0 = blockIdx.x * 64;
  const float* s = src + (size_t)b * kC * HW;
  float4* d = reinterpret_cast<float4*>(dst + (size_t)b * kC * HW);
  const int px = threadIdx.x & 63;
  float mx = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = (threadIdx.x >> 6) + 4 * j;
    const float v = p0 + px < HW ? s[(size_t)c * HW + p0 + px] : 0.f;
    t[c][px] = v;
    // NaN-propagating max of |v| (a NaN feature forces the largest fp16 guard scale)
    const float av = fabsf(v);
    mx = (av > mx || av != av) ? av : mx;
  }
  if (xbound) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float q = __shfl_xor(mx, o, 64);
      mx = (q > mx || q != q) ? q : mx;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (xbound && threadIdx.x == 0) {
    float m = 0.f;
    for (int w = 0; w < 4; ++w) m = (wmax[w] > m || wmax[w] != wmax[w]) ? wmax[w] : m;
    const float bound = 8.0f * m * m;   // non-negative: float bits order like unsigned
    const unsigned bits = __float_as_uint(bound != bound ? INFINITY : bound);
    // one address for the whole grid: read first, so that only blocks that raise the bound
    // pay a (serialised) atomic
    if (bits > __hip_atomic_load(xbound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(xbound, bits);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = threadIdx.x + 256 * j, ch = idx >> 7, q = (idx & 127) >> 1, h = idx & 1;
    const int c0 = 8 * ch + 4 * h;
    if (p0 + q < HW)
      d[((size_t)ch * HW + p0 + q) * 2 + h] =
          make_float4(t[c0][q], t[c0 + 1][q], t[c0 + 2][q], t[c0 + 3][q]);
  }
}

hipError_t launch_to_c8(const float* src, float* dst, int B, int HW, hipStream_t s,
                        unsigned* xbound) {
  ProfScope ps(s, K_TO_C8);
  hipLaunchKernelGGL(nchw_to_c8_kernel, dim3((HW + 63) / 64, B), dim3(256), 0, s, src, dst, HW,
                     xbound);
  return hipGetLastError();
}

}  // namespace aarmvs
