// Depth head of the recurrent regulariser (models/drmvsnet.py:117, 165, 324-334) for gfx950:
// the conv_0 head fused with the online winner-take-all, its sub-plane refinement and
// posterior statistics, their stand-alone and from-the-volume forms, the final depth and
// confidence, the softmax depth and the NCHW <-> NHWC layout kernel.
#include <hip/hip_runtime.h>

#include <cfloat>

#include <algorithm>

#include "device_common.h"

namespace aarmvs {

// ---------------------------------------------------------------------------
// conv_0 head (drmvsnet.py:117,165: Conv2d(8,1,3,pad 1)) fused with the online
// winner-take-all update (drmvsnet.py:324-334) and the optional cost-volume store.
// ---------------------------------------------------------------------------
constexpr int kHeadTH = 8, kHeadTW = 32;

// drmvsnet.py:324-334 for one pixel: p = exp(cost) (no max-subtraction), strict-< flag,
// the arithmetic select of max_prob and depth, exp_sum += p -- op for op (contract off)
__device__ __forceinline__ void wta_select(float cost, float dv, float& max_prob, float& depth,
                                           float& exp_sum) {
#pragma clang fp contract(off)
  const float pr = expf(cost);
  const float mp = max_prob;
  const float f = (mp < pr) ? 1.0f : 0.0f;
  max_prob = __fadd_rn(__fmul_rn(f, pr), __fmul_rn(1.0f - f, mp));
  depth = __fadd_rn(__fmul_rn(f, dv), __fmul_rn(1.0f - f, depth));
  exp_sum = __fadd_rn(exp_sum, pr);
}

// ---------------------------------------------------------------------------
// Sub-plane refinement of the winner-take-all (opt-in, beyond the reference).
// Per pixel, beside the WTA images: the winner's plane index and the probabilities of the planes
// next to it, kept online (16 B per pixel in a caller-owned buffer).  The head kernel, the
// standalone per-plane pair and the from-the-volume kernel all go through refine_step /
// refine_finish, so they agree bit for bit on the same cost values.
// ---------------------------------------------------------------------------
struct RefineState {
  int idx;                       // the winner's plane, -1 while no plane has won
  float p_prev, p_left, p_right; // p of the last plane seen; p of the planes idx - 1 and idx + 1
};
static_assert(sizeof(RefineState) == 16, "aarmvs_refine_state_bytes is 16 B per pixel");

__device__ __forceinline__ RefineState refine_load(const void* state, size_t q) {
  const int4 v = reinterpret_cast<const int4*>(state)[q];
  return {v.x, __int_as_float(v.y), __int_as_float(v.z), __int_as_float(v.w)};
}
__device__ __forceinline__ void refine_store(void* state, size_t q, const RefineState& r) {
  reinterpret_cast<int4*>(state)[q] =
      make_int4(r.idx, __float_as_int(r.p_prev), __float_as_int(r.p_left), __float_as_int(r.p_right));
}

// plane d's update, from the plane's cost and max_prob BEFORE wta_select: p and the flag are
// the values wta_select forms (expf of the same cost, the strict <)
__device__ __forceinline__ void refine_step(float cost, int d, float max_prob_before, RefineState& r) {
  const float p = expf(cost);
  if (max_prob_before < p) {
    r.idx = d;
    r.p_left = r.p_prev;
    r.p_right = 0.0f;
  } else if (r.idx == d - 1) {
    r.p_right = p;
  }
  r.p_prev = p;
}

// the three outputs of one pixel after n planes; dv: the batch element's depth_values [D];
// max_prob / exp_sum / depth: the WTA images' values (max_prob is p of the winner)
__device__ __forceinline__ void refine_finish(const RefineState& r, float max_prob, float exp_sum,
                                              float depth, const float* __restrict__ dv, int n,
                                              float& depth_refined, float& conf_window) {
#pragma clang fp contract(off)
  const int w = r.idx;
  depth_refined = depth;
  if (w < 0) {
    conf_window = __fdiv_rn(max_prob, exp_sum);
    return;
  }
  const bool left = w >= 1, right = w + 1 < n;
  const float pl = left ? r.p_left : 0.0f, pr = right ? r.p_right : 0.0f;
  const float s = __fadd_rn(__fadd_rn(pl, max_prob), pr);
  conf_window = __fdiv_rn(s, exp_sum);
  if (left && right) {
    const float dw = dv[w];
    const float num = __fadd_rn(__fmul_rn(pl, __fsub_rn(dv[w - 1], dw)),
                                __fmul_rn(pr, __fsub_rn(dv[w + 1], dw)));
    if (isfinite(s) && isfinite(num)) depth_refined = __fadd_rn(dw, __fdiv_rn(num, s));
  }
}

// ---------------------------------------------------------------------------
// Depth-posterior statistics of the sweep (opt-in, beyond the reference): the
// softmax-weighted mean and variance of depth, the weighted mean cost (for the entropy) and the
// runner-up probability, kept online beside the WTA images (16 B per pixel in a caller-owned
// buffer).  The head kernel, the standalone per-plane pair and the from-the-volume kernel all go
// through posterior_step / posterior_finish, so they agree bit for bit on the same cost values.
// ---------------------------------------------------------------------------
struct PosteriorState {
  float mu, var, ecost, p2;   // weighted mean depth, weighted variance, weighted mean cost, runner-up p
};
static_assert(sizeof(PosteriorState) == 16, "aarmvs_posterior_state_bytes is 16 B per pixel");

__device__ __forceinline__ PosteriorState posterior_load(const void* state, size_t q) {
  const float4 v = reinterpret_cast<const float4*>(state)[q];
  return {v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void posterior_store(void* state, size_t q, const PosteriorState& r) {
  reinterpret_cast<float4*>(state)[q] = make_float4(r.mu, r.var, r.ecost, r.p2);
}

// plane d's update from the plane's cost, its depth value, and max_prob / exp_sum BEFORE
// wta_select: p and S1 are the values wta_select forms.  The variance is rescaled by S0 / S1, not
// by 1 - k: with a dominant plane k rounds to within an ulp of 1 and 1 - k has no correct digit.
// Plain operators under contract(off), not __fmul_rn / __fadd_rn: this toolchain's headers define
// those as x * y and x + y in a scope the pragma does not reach, so a product and a sum written
// with them may still fuse, differently from one kernel to the next.
__device__ __forceinline__ void posterior_step(float cost, float x, float max_prob_before,
                                               float exp_sum_before, PosteriorState& r) {
#pragma clang fp contract(off)
  const float p = expf(cost);
  if (max_prob_before < p) r.p2 = max_prob_before;
  else if (r.p2 < p) r.p2 = p;
  if (p > 0.0f) {
    const float s1 = exp_sum_before + p;
    const float k = p / s1, j = exp_sum_before / s1;
    const float dl = x - r.mu;
    const float dk = dl * k, d2 = dl * dl, ck = (cost - r.ecost) * k;
    const float d2k = d2 * k;
    r.mu = r.mu + dk;
    r.var = j * (r.var + d2k);
    r.ecost = r.ecost + ck;
  }
}

// the four outputs of one pixel from the state and the WTA image's exp_sum
__device__ __forceinline__ void posterior_finish(const PosteriorState& r, float exp_sum, float& mean,
                                                 float& sd, float& entropy, float& runner_up) {
#pragma clang fp contract(off)
  if (!(exp_sum > 0.0f && isfinite(exp_sum))) {
    mean = sd = entropy = runner_up = __int_as_float(0x7fc00000);
    return;
  }
  mean = r.mu;
  sd = sqrtf(r.var);
  const float h = logf(exp_sum) - r.ecost;
  entropy = h > 0.0f ? h : 0.0f;
  runner_up = r.p2 / exp_sum;
}

// aarmvs_wta_update: the online WTA of one plane on a caller-given cost slice [B,HW]
__global__ void __launch_bounds__(256) wta_update_kernel(const float* __restrict__ cost,
                                                         const float* __restrict__ depth_d,
                                                         float* __restrict__ max_prob,
                                                         float* __restrict__ depth,
                                                         float* __restrict__ exp_sum, int HW) {
  const int b = blockIdx.y;
  const float dv = depth_d[b];
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const size_t q = (size_t)b * HW + p;
    float mp = max_prob[q], dp = depth[q], es = exp_sum[q];
    wta_select(cost[q], dv, mp, dp, es);
    max_prob[q] = mp;
    depth[q] = dp;
    exp_sum[q] = es;
  }
}

static hipError_t launch_wta_update(const float* cost, const float* depth_d, float* max_prob,
                                    float* depth, float* exp_sum, int B, int HW, hipStream_t s) {
  const int blocks = std::max(1, std::min((HW + 255) / 256, 4096));
  ProfScope ps(s, K_HEAD_WTA);
  hipLaunchKernelGGL(wta_update_kernel, dim3(blocks, B), dim3(256), 0, s, cost, depth_d, max_prob,
                     depth, exp_sum, HW);
  return hipGetLastError();
}

// The haloed h4 tile sits in LDS pixel-major (32 B per pixel, the NHWC layout): a pixel's 9
// taps are 18 ds_read_b128 (the fma order stays channel-major, tap-minor), the staging 2 16-B
// stores per pixel (27.8 vs 28.8 us per plane at the headline against a channel-major tile
// read by 72 scalar LDS loads; bit-identical).
// REFINE: the sweep's refining variant also carries the sub-plane state (loaded with the WTA
// state, stored with it); the default instantiation has no trace of it.
// POST: likewise the depth-posterior state (posterior_step), independent of REFINE.
template <bool REFINE, bool POST>
__global__ void __launch_bounds__(256) head_wta_kernel(const float* __restrict__ h4,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ bias, int H,
                                                        int W, const float* __restrict__ dvals,
                                                        int d, int D, float* __restrict__ cost_out,
                                                        int wta, float* __restrict__ max_prob,
                                                        float* __restrict__ exp_sum,
                                                        float* __restrict__ depth,
                                                        double* __restrict__ zero_stats,
                                                        int zero_n, void* __restrict__ refine,
                                                        void* __restrict__ posterior) {
#pragma clang fp contract(off)
  constexpr int TW2 = kHeadTW + 2, NPX = (kHeadTH + 2) * TW2;
  __shared__ float4 t[NPX][2];
  if (zero_stats && blockIdx.x == 0 && blockIdx.y == 0)
    for (int i = threadIdx.x; i < zero_n; i += blockDim.x) zero_stats[i] = 0.0;
  const int b = blockIdx.y, HW = H * W;
  const int tiles_x = (W + kHeadTW - 1) / kHeadTW;
  const int y0 = (blockIdx.x / tiles_x) * kHeadTH, x0 = (blockIdx.x % tiles_x) * kHeadTW;
  const float* hb = h4 + (size_t)b * 8 * HW;
  // this thread's pixel and its WTA state, loaded with the tile (one memory round trip, not a
  // second one after the conv)
  const int ty = threadIdx.x / kHeadTW, tx = threadIdx.x % kHeadTW;
  const int y = y0 + ty, x = x0 + tx;
  const bool own = y < H && x < W;
  const int p = own ? y * W + x : 0;
  const size_t q = (size_t)b * HW + p;
  float mp = 0.f, dp = 0.f, es = 0.f;
  if (wta && own) {
    mp = max_prob[q];
    dp = depth[q];
    es = exp_sum[q];
  }
  RefineState rs{-1, 0.f, 0.f, 0.f};   // plane 0 starts from the reset state
  if constexpr (REFINE) {
    if (wta && own && d > 0) rs = refine_load(refine, q);
  }
  PosteriorState ps{0.f, 0.f, 0.f, 0.f};   // plane 0 starts from all zeros
  if constexpr (POST) {
    if (wta && own && d > 0) ps = posterior_load(posterior, q);
  }
  for (int rem = threadIdx.x; rem < NPX; rem += 256) {
    const int yy = y0 - 1 + rem / TW2, xx = x0 - 1 + rem % TW2;
    float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      const float4* src = reinterpret_cast<const float4*>(hb + ((size_t)yy * W + xx) * 8);
      q0 = src[0];
      q1 = src[1];
    }
    t[rem][0] = q0;
    t[rem][1] = q1;
  }
  __syncthreads();
  if (!own) return;
  float v[9][8];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int qt = (ty + tap / 3) * TW2 + tx + tap % 3;
    const float4 a0 = t[qt][0], a1 = t[qt][1];
    v[tap][0] = a0.x; v[tap][1] = a0.y; v[tap][2] = a0.z; v[tap][3] = a0.w;
    v[tap][4] = a1.x; v[tap][5] = a1.y; v[tap][6] = a1.z; v[tap][7] = a1.w;
  }
  float acc = 0.f;
#pragma unroll
  for (int ci = 0; ci < 8; ++ci)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc = fmaf(v[tap][ci], w[ci * 9 + tap], acc);
  const float cost = acc + bias[0];
  if (cost_out) cost_out[((size_t)b * D + d) * HW + p] = cost;
  if (wta) {
    if constexpr (REFINE) refine_step(cost, d, mp, rs);
    if constexpr (POST) posterior_step(cost, dvals[b * D + d], mp, es, ps);
    wta_select(cost, dvals[b * D + d], mp, dp, es);
    max_prob[q] = mp;
    depth[q] = dp;
    exp_sum[q] = es;
    if constexpr (REFINE) refine_store(refine, q, rs);
    if constexpr (POST) posterior_store(posterior, q, ps);
  }
}

__global__ void finalize_kernel(const float* __restrict__ max_prob, const float* __restrict__ exp_sum,
                                const float* __restrict__ depth, size_t n, float* depth_out,
                                float* conf_out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    if (depth_out) depth_out[i] = depth[i];
    if (conf_out) conf_out[i] = __fdiv_rn(max_prob[i], exp_sum[i]);
  }
}

// the refining finalize: depth_refined / conf_window / index of B*HW pixels after n planes
__global__ void __launch_bounds__(256) refine_finalize_kernel(
    const float* __restrict__ max_prob, const float* __restrict__ exp_sum,
    const float* __restrict__ depth, const void* __restrict__ state,
    const float* __restrict__ dvals, int D, int n, int HW, float* __restrict__ depth_refined,
    float* __restrict__ conf_window, int* __restrict__ index) {
  const int b = blockIdx.y;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const size_t q = (size_t)b * HW + p;
    const RefineState rs = refine_load(state, q);
    float dr, cw;
    refine_finish(rs, max_prob[q], exp_sum[q], depth[q], dvals + (size_t)b * D, n, dr, cw);
    if (depth_refined) depth_refined[q] = dr;
    if (conf_window) conf_window[q] = cw;
    if (index) index[q] = rs.idx;
  }
}

// aarmvs_wta_refine_update: aarmvs_wta_update of plane d plus the sub-plane state, on a
// caller-given cost slice [B,HW]; d == 0 starts from the reset state
__global__ void __launch_bounds__(256) wta_refine_update_kernel(
    const float* __restrict__ cost, const float* __restrict__ depth_d, int d,
    float* __restrict__ max_prob, float* __restrict__ depth, float* __restrict__ exp_sum,
    void* __restrict__ state, int HW) {
  const int b = blockIdx.y;
  const float dv = depth_d[b];
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const size_t q = (size_t)b * HW + p;
    float mp = max_prob[q], dp = depth[q], es = exp_sum[q];
    RefineState rs{-1, 0.f, 0.f, 0.f};
    if (d != 0) rs = refine_load(state, q);
    const float c = cost[q];
    refine_step(c, d, mp, rs);
    wta_select(c, dv, mp, dp, es);
    max_prob[q] = mp;
    depth[q] = dp;
    exp_sum[q] = es;
    refine_store(state, q, rs);
  }
}

// aarmvs_refine_from_cost: the same over a whole cost volume [B,D,HW], one thread per
// (b, pixel), coalesced over pixels; the WTA images and the state stay in registers
__global__ void __launch_bounds__(256) refine_from_cost_kernel(
    const float* __restrict__ cost, const float* __restrict__ dvals, int D, int HW,
    float* __restrict__ depth_refined, float* __restrict__ conf_window, int* __restrict__ index) {
  const int b = blockIdx.y;
  const float* dv = dvals + (size_t)b * D;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const float* c = cost + (size_t)b * D * HW + p;
    float mp = 0.f, dp = 0.f, es = 0.f;
    RefineState rs{-1, 0.f, 0.f, 0.f};
    for (int d = 0; d < D; ++d) {
      const float v = c[(size_t)d * HW];
      refine_step(v, d, mp, rs);
      wta_select(v, dv[d], mp, dp, es);
    }
    const size_t q = (size_t)b * HW + p;
    float dr, cw;
    refine_finish(rs, mp, es, dp, dv, D, dr, cw);
    if (depth_refined) depth_refined[q] = dr;
    if (conf_window) conf_window[q] = cw;
    if (index) index[q] = rs.idx;
  }
}

// the posterior finalize: mean / std / entropy / runner_up of B*HW pixels from the state and exp_sum
__global__ void __launch_bounds__(256) posterior_finalize_kernel(
    const float* __restrict__ exp_sum, const void* __restrict__ state, int HW,
    float* __restrict__ mean, float* __restrict__ sd, float* __restrict__ entropy,
    float* __restrict__ runner_up) {
  const int b = blockIdx.y;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const size_t q = (size_t)b * HW + p;
    float m, s, h, r2;
    posterior_finish(posterior_load(state, q), exp_sum[q], m, s, h, r2);
    if (mean) mean[q] = m;
    if (sd) sd[q] = s;
    if (entropy) entropy[q] = h;
    if (runner_up) runner_up[q] = r2;
  }
}

// aarmvs_wta_posterior_update: aarmvs_wta_update of plane d plus the posterior state, on a
// caller-given cost slice [B,HW]; d == 0 starts from the all-zero state
__global__ void __launch_bounds__(256) wta_posterior_update_kernel(
    const float* __restrict__ cost, const float* __restrict__ depth_d, int d,
    float* __restrict__ max_prob, float* __restrict__ depth, float* __restrict__ exp_sum,
    void* __restrict__ state, int HW) {
  const int b = blockIdx.y;
  const float dv = depth_d[b];
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const size_t q = (size_t)b * HW + p;
    float mp = max_prob[q], dp = depth[q], es = exp_sum[q];
    PosteriorState ps{0.f, 0.f, 0.f, 0.f};
    if (d != 0) ps = posterior_load(state, q);
    const float c = cost[q];
    posterior_step(c, dv, mp, es, ps);
    wta_select(c, dv, mp, dp, es);
    max_prob[q] = mp;
    depth[q] = dp;
    exp_sum[q] = es;
    posterior_store(state, q, ps);
  }
}

// aarmvs_posterior_from_cost: the same over a whole cost volume [B,D,HW], one thread per
// (b, pixel), coalesced over pixels; the WTA images and the state stay in registers
__global__ void __launch_bounds__(256) posterior_from_cost_kernel(
    const float* __restrict__ cost, const float* __restrict__ dvals, int D, int HW,
    float* __restrict__ mean, float* __restrict__ sd, float* __restrict__ entropy,
    float* __restrict__ runner_up) {
  const int b = blockIdx.y;
  const float* dv = dvals + (size_t)b * D;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const float* c = cost + (size_t)b * D * HW + p;
    float mp = 0.f, dp = 0.f, es = 0.f;
    PosteriorState ps{0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < D; ++d) {
      const float v = c[(size_t)d * HW];
      posterior_step(v, dv[d], mp, es, ps);
      wta_select(v, dv[d], mp, dp, es);
    }
    const size_t q = (size_t)b * HW + p;
    float m, s, h, r2;
    posterior_finish(ps, es, m, s, h, r2);
    if (mean) mean[q] = m;
    if (sd) sd[q] = s;
    if (entropy) entropy[q] = h;
    if (runner_up) runner_up[q] = r2;
  }
}

// softmax over D (dim=1 of [B,D,H,W], drmvsnet.py:291/:342); one thread per (b, pixel),
// coalesced over pixels.  Two passes over D instead of three: the running max and the
// rescaled running sum in one (online softmax, one exp per element: e = exp(-|v - m|)
// serves both the rescale of the sum when v raises the max and the new term otherwise),
// then exp(v - m) / sum.  Four planes' loads in flight per iteration.
// Non-finite columns come out as torch.softmax's three passes give them: the running max starts
// at -FLT_MAX, not -inf, so a -inf cost is a term of exactly 0 (v - m = -inf, not -inf + inf =
// NaN) and a column of nothing but -inf is 0 * (1 / 0) = NaN; an infinite final max adds m - m =
// NaN to the sum, which is what the three-pass form's own exp(m - m) term does.  For a finite
// column m - m = 0 and every bit is as before.
__global__ void __launch_bounds__(256) softmax_depth_kernel(const float* __restrict__ cost,
                                                            float* __restrict__ prob, int D,
                                                            int HW) {
  const int b = blockIdx.y;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const float* c = cost + (size_t)b * D * HW + p;
    float* o = prob + (size_t)b * D * HW + p;
    float m = -FLT_MAX, s = 0.f;
    auto add = [&](float v) {
      const float dv = v - m;
      const float e = expf(-fabsf(dv));
      if (dv > 0.f) {
        s = s * e + 1.0f;
        m = v;
      } else {
        s += e;
      }
    };
    int d = 0;
    for (; d + 4 <= D; d += 4) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = c[(size_t)(d + u) * HW];
#pragma unroll
      for (int u = 0; u < 4; ++u) add(v[u]);
    }
    for (; d < D; ++d) add(c[(size_t)d * HW]);
    const float inv = 1.0f / (s + (m - m));
    for (d = 0; d + 4 <= D; d += 4) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = c[(size_t)(d + u) * HW];
#pragma unroll
      for (int u = 0; u < 4; ++u) o[(size_t)(d + u) * HW] = expf(v[u] - m) * inv;
    }
    for (; d < D; ++d) o[(size_t)d * HW] = expf(c[(size_t)d * HW] - m) * inv;
  }
}

// NCHW <-> NHWC for the API edges (aarmvs_unet_step's input slice, the debug slice copy):
// one thread per (b, pixel), all channels.
__global__ void __launch_bounds__(256) layout_kernel(const float* __restrict__ in,
                                                     float* __restrict__ out, int C, int HW,
                                                     int to_nhwc, unsigned* __restrict__ xmax) {
  const int b = blockIdx.y;
  const float* ib = in + (size_t)b * C * HW;
  float* ob = out + (size_t)b * C * HW;
  float mx = 0.f;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x)
    for (int c = 0; c < C; ++c) {
      if (to_nhwc) {
        const float v = ib[(size_t)c * HW + p];
        ob[(size_t)p * C + c] = v;
        const float av = fabsf(v);
        mx = (av > mx || av != av) ? av : mx;
      } else {
        ob[(size_t)c * HW + p] = ib[(size_t)p * C + c];
      }
    }
  if (xmax) {   // |x| bound for cell 0's fp16 range guard (one atomic per wave)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float q = __shfl_xor(mx, o, 64);
      mx = (q > mx || q != q) ? q : mx;
    }
    const unsigned bits = __float_as_uint(mx != mx ? INFINITY : mx);
    if ((threadIdx.x & 63) == 0 &&
        bits > __hip_atomic_load(xmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(xmax, bits);
  }
}

hipError_t launch_layout(const float* in, float* out, int B, int C, int HW, bool to_nhwc,
                         hipStream_t s, unsigned* xmax) {
  const int blocks = std::max(1, std::min((HW + 255) / 256, 4096));
  hipLaunchKernelGGL(layout_kernel, dim3(blocks, B), dim3(256), 0, s, in, out, C, HW,
                     to_nhwc ? 1 : 0, to_nhwc ? xmax : nullptr);
  return hipGetLastError();
}

hipError_t launch_head_wta(const float* params, const SweepGeom& g, const UnetIO& io,
                           const Workspace& ws, const float* depth_values, int d,
                           float* cost_out, bool wta, hipStream_t s, void* refine_state,
                           void* posterior_state) {
  const ParamLayout& L = param_layout();
  const int blocks = ((g.W + kHeadTW - 1) / kHeadTW) * ((g.H + kHeadTH - 1) / kHeadTH);
  ProfScope ps(s, K_HEAD_WTA);
  auto kernel = refine_state ? (posterior_state ? head_wta_kernel<true, true> : head_wta_kernel<true, false>)
                             : (posterior_state ? head_wta_kernel<false, true> : head_wta_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks, g.B), dim3(256), 0, s, io.h_new[4],
                     params + L.pk_off[P_HW], params + L.pk_off[P_HB], g.H, g.W, depth_values, d,
                     g.D, cost_out, wta ? 1 : 0, ws.max_prob, ws.exp_sum, ws.depth,
                     io.clear_stats ? io.reg_stats : nullptr,
                     (int)(ws.reg_stats_bytes / sizeof(double)), refine_state, posterior_state);
  return hipGetLastError();
}

hipError_t launch_finalize(const SweepGeom& g, const Workspace& ws, float* depth_out,
                           float* conf_out, hipStream_t s) {
  const size_t n = (size_t)g.B * g.H * g.W;
  const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
  ProfScope ps(s, K_FINALIZE);
  hipLaunchKernelGGL(finalize_kernel, dim3(blocks), dim3(256), 0, s, ws.max_prob, ws.exp_sum,
                     ws.depth, n, depth_out, conf_out);
  return hipGetLastError();
}

hipError_t launch_refine_finalize(const float* max_prob, const float* exp_sum, const float* depth,
                                  const void* state, const float* depth_values, int B, int D, int n,
                                  int HW, float* depth_refined, float* conf_window, int* index,
                                  hipStream_t s) {
  const int blocks = std::max(1, std::min((HW + 255) / 256, 4096));
  ProfScope ps(s, K_REFINE);
  hipLaunchKernelGGL(refine_finalize_kernel, dim3(blocks, B), dim3(256), 0, s, max_prob, exp_sum,
                     depth, state, depth_values, D, n, HW, depth_refined, conf_window, index);
  return hipGetLastError();
}

static hipError_t launch_wta_refine_update(const float* cost, const float* depth_d, int d, float* max_prob,
                                           float* depth, float* exp_sum, void* state, int B, int HW,
                                           hipStream_t s) {
  const int blocks = std::max(1, std::min((HW + 255) / 256, 4096));
  ProfScope ps(s, K_HEAD_WTA);
  hipLaunchKernelGGL(wta_refine_update_kernel, dim3(blocks, B), dim3(256), 0, s, cost, depth_d, d,
                     max_prob, depth, exp_sum, state, HW);
  return hipGetLastError();
}

static hipError_t launch_refine_from_cost(const float* cost, const float* depth_values, int B, int D, int HW,
                                          float* depth_refined, float* conf_window, int* index,
                                          hipStream_t s) {
  const int blocks = std::max(1, std::min((HW + 255) / 256, 4096));
  ProfScope ps(s, K_REFINE);
  hipLaunchKernelGGL(refine_from_cost_kernel, dim3(blocks, B), dim3(256), 0, s, cost, depth_values,
                     D, HW, depth_refined, conf_window, index);
  return hipGetLastError();
}

hipError_t launch_posterior_finalize(const float* exp_sum, const void* state, int B, int HW,
                                     float* mean, float* sd, float* entropy, float* runner_up,
                                     hipStream_t s) {
  const int blocks = std::max(1, std::min((HW + 255) / 256, 4096));
  ProfScope ps(s, K_REFINE);
  hipLaunchKernelGGL(posterior_finalize_kernel, dim3(blocks, B), dim3(256), 0, s, exp_sum, state, HW,
                     mean, sd, entropy, runner_up);
  return hipGetLastError();
}

static hipError_t launch_wta_posterior_update(const float* cost, const float* depth_d, int d, float* max_prob,
                                              float* depth, float* exp_sum, void* state, int B, int HW,
                                              hipStream_t s) {
  const int blocks = std::max(1, std::min((HW + 255) / 256, 4096));
  ProfScope ps(s, K_HEAD_WTA);
  hipLaunchKernelGGL(wta_posterior_update_kernel, dim3(blocks, B), dim3(256), 0, s, cost, depth_d, d,
                     max_prob, depth, exp_sum, state, HW);
  return hipGetLastError();
}

static hipError_t launch_posterior_from_cost(const float* cost, const float* depth_values, int B, int D,
                                             int HW, float* mean, float* sd, float* entropy,
                                             float* runner_up, hipStream_t s) {
  const int blocks = std::max(1, std::min((HW + 255) / 256, 4096));
  ProfScope ps(s, K_REFINE);
  hipLaunchKernelGGL(posterior_from_cost_kernel, dim3(blocks, B), dim3(256), 0, s, cost, depth_values,
                     D, HW, mean, sd, entropy, runner_up);
  return hipGetLastError();
}

static hipError_t launch_softmax_depth(const float* cost, float* prob, int B, int D, int HW,
                                       hipStream_t s) {
  const int blocks = std::max(1, std::min((HW + 255) / 256, 4096));
  ProfScope ps(s, K_SOFTMAX);
  hipLaunchKernelGGL(softmax_depth_kernel, dim3(blocks, B), dim3(256), 0, s, cost, prob, D, HW);
  return hipGetLastError();
}

}  // namespace aarmvs

using namespace aarmvs;

extern "C" {

size_t aarmvs_posterior_state_bytes(int B, int HW) {
  if (B < 1 || HW < 1) return 0;
  return (size_t)16 * B * HW;
}

size_t aarmvs_refine_state_bytes(int B, int HW) {
  if (B < 1 || HW < 1) return 0;
  return (size_t)16 * B * HW;
}

int aarmvs_wta_update(const float* cost, const float* depth_d, float* max_prob, float* depth_map,
                      float* exp_sum, int B, int HW, hipStream_t stream) {
  if (!cost || !depth_d || !max_prob || !depth_map || !exp_sum || B < 1 || HW < 1)
    return fail(AARMVS_ERR_INVALID, "wta_update: bad arguments");
  return launched(launch_wta_update(cost, depth_d, max_prob, depth_map, exp_sum, B, HW, stream), "wta_update");
}

int aarmvs_wta_refine_update(const float* cost, int d, float* max_prob, float* depth_map,
                             float* exp_sum, void* state, const float* depth_d, int B, int HW,
                             hipStream_t stream) {
  if (!cost || !depth_d || !max_prob || !depth_map || !exp_sum || !state || B < 1 || HW < 1 || d < 0)
    return fail(AARMVS_ERR_INVALID, "wta_refine_update: bad arguments");
  return launched(launch_wta_refine_update(cost, depth_d, d, max_prob, depth_map, exp_sum, state, B, HW, stream),
                  "wta_refine_update");
}

int aarmvs_wta_refine_finalize(const float* max_prob, const float* depth_map, const float* exp_sum,
                               const void* state, const float* depth_values, int B, int D, int n,
                               int HW, float* depth_refined, float* conf_window, int* index,
                               hipStream_t stream) {
  if (!max_prob || !depth_map || !exp_sum || !state || !depth_values)
    return fail(AARMVS_ERR_INVALID, "wta_refine_finalize: null pointer argument");
  if (B < 1 || HW < 1 || D < 1 || n < 1 || n > D)
    return fail(AARMVS_ERR_INVALID, "wta_refine_finalize: need B, HW >= 1 and 1 <= n <= D");
  return launched(launch_refine_finalize(max_prob, exp_sum, depth_map, state, depth_values, B, D, n, HW,
                                         depth_refined, conf_window, index, stream),
                  "wta_refine_finalize");
}

int aarmvs_refine_from_cost(const float* cost, const float* depth_values, int B, int D, int HW,
                            float* depth_refined, float* conf_window, int* index, hipStream_t stream) {
  if (!cost || !depth_values)
    return fail(AARMVS_ERR_INVALID, "refine_from_cost: null pointer argument");
  if (B < 1 || D < 1 || HW < 1)
    return fail(AARMVS_ERR_INVALID, "refine_from_cost: need B, D, HW >= 1");
  return launched(launch_refine_from_cost(cost, depth_values, B, D, HW, depth_refined, conf_window, index, stream),
                  "refine_from_cost");
}

int aarmvs_wta_posterior_update(const float* cost, int d, float* max_prob, float* depth_map,
                                float* exp_sum, void* state, const float* depth_d, int B, int HW,
                                hipStream_t stream) {
  if (!cost || !depth_d || !max_prob || !depth_map || !exp_sum || !state || B < 1 || HW < 1 || d < 0)
    return fail(AARMVS_ERR_INVALID, "wta_posterior_update: bad arguments");
  return launched(launch_wta_posterior_update(cost, depth_d, d, max_prob, depth_map, exp_sum, state, B, HW, stream),
                  "wta_posterior_update");
}

int aarmvs_wta_posterior_finalize(const float* exp_sum, const void* state, int B, int HW, float* mean,
                                  float* std_out, float* entropy, float* runner_up, hipStream_t stream) {
  if (!exp_sum || !state) return fail(AARMVS_ERR_INVALID, "wta_posterior_finalize: null pointer argument");
  if (B < 1 || HW < 1) return fail(AARMVS_ERR_INVALID, "wta_posterior_finalize: need B, HW >= 1");
  return launched(launch_posterior_finalize(exp_sum, state, B, HW, mean, std_out, entropy, runner_up, stream),
                  "wta_posterior_finalize");
}

int aarmvs_posterior_from_cost(const float* cost, const float* depth_values, int B, int D, int HW,
                               float* mean, float* std_out, float* entropy, float* runner_up,
                               hipStream_t stream) {
  if (!cost || !depth_values)
    return fail(AARMVS_ERR_INVALID, "posterior_from_cost: null pointer argument");
  if (B < 1 || D < 1 || HW < 1)
    return fail(AARMVS_ERR_INVALID, "posterior_from_cost: need B, D, HW >= 1");
  return launched(launch_posterior_from_cost(cost, depth_values, B, D, HW, mean, std_out, entropy, runner_up, stream),
                  "posterior_from_cost");
}

int aarmvs_softmax_depth(const float* cost, float* prob, int B, int D, int HW, hipStream_t stream) {
  if (!cost || !prob || B < 1 || D < 1 || HW < 1)
    return fail(AARMVS_ERR_INVALID, "softmax_depth: bad arguments");
  return launched(launch_softmax_depth(cost, prob, B, D, HW, stream), "softmax_depth");
}

}  // extern "C"
