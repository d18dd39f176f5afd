// Stand-alone homography warp (aarmvs_homo_warp) and its backward for gfx950.
//
// Reference: models/module.py:6-38 (homo_warping_depthwise).
#include <hip/hip_runtime.h>

#include <cfloat>

#include "cost_device.h"

namespace aarmvs {

// Bilinear taps with zero padding.  Invalid taps get index 0 and weight 0.
struct Taps {
  unsigned idx[4];
  float wt[4];
  bool ok[4];
};

__device__ __forceinline__ Taps make_taps(float ix, float iy, int H, int W) {
  Taps t;
  const float x0 = floorf(ix), y0 = floorf(iy);
  const float wx = __fsub_rn(ix, x0), wy = __fsub_rn(iy, y0);
  const float ex = __fsub_rn(1.0f, wx), sy = __fsub_rn(1.0f, wy);
  const float wts[4] = {__fmul_rn(sy, ex), __fmul_rn(sy, wx), __fmul_rn(wy, ex), __fmul_rn(wy, wx)};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float xf = x0 + (float)(k & 1), yf = y0 + (float)(k >> 1);
    const bool ok = (xf > -1.0f) && (xf < (float)W) && (yf > -1.0f) && (yf < (float)H);
    t.ok[k] = ok;
    t.idx[k] = ok ? (unsigned)((int)yf * W + (int)xf) : 0u;
    t.wt[k] = wts[k];
  }
  return t;
}

__device__ __forceinline__ float bilinear(const float* __restrict__ plane, const Taps& t) {
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = t.ok[k] ? plane[t.idx[k]] : 0.0f;
  // nw*wnw + ne*wne + sw*wsw + se*wse as the compiled ATen CPU kernel evaluates it
  // (left to right, contracted into an fma chain)
  return __fmaf_rn(v[3], t.wt[3],
                   __fmaf_rn(v[2], t.wt[2], __fmaf_rn(v[1], t.wt[1], __fmul_rn(v[0], t.wt[0]))));
}


// ---------------------------------------------------------------------------
// Standalone warp (aarmvs_homo_warp): one thread per (b, pixel), all channels.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) homo_warp_kernel(const float* __restrict__ src,
                                                        const float* __restrict__ rel,
                                                        const float* __restrict__ depth, int C,
                                                        int H, int W, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int HW = H * W;
  const float* m = rel + 12 * b;
  const float dep = depth[b];
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    float ix, iy;
    sample_pos(m, dep, (float)(p % W), (float)(p / W), H, W, ix, iy);
    const Taps t = make_taps(ix, iy, H, W);
    const float* s = src + (size_t)b * C * HW;
    float* o = out + (size_t)b * C * HW + p;
    for (int c = 0; c < C; ++c) o[(size_t)c * HW] = bilinear(s + (size_t)c * HW, t);
  }
}

static hipError_t launch_homo_warp(const float* src, const float* rel, const float* depth, int B, int C,
                                   int H, int W, float* out, hipStream_t s) {
  const int HW = H * W;
  dim3 grid((unsigned)std::min((HW + 255) / 256, 4096), (unsigned)B);
  ProfScope ps(s, K_WARP);
  hipLaunchKernelGGL(homo_warp_kernel, grid, dim3(256), 0, s, src, rel, depth, C, H, W, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Backward of the warp w.r.t. the source features (aarmvs_homo_warp_backward, the gradient of
// grid_sample at module.py:36): a scatter-add of the output gradient into the four bilinear
// taps, many reference pixels into one source pixel.  fp32 atomics would make each sum depend on
// the order the atomics are served in, so the sums are formed in 64-bit fixed point instead
// (integer adds are associative: bit-reproducible), as the sweep's own dL/dsrc (cbw_feat):
//   1. warp_bwd_max: max |grad_out| per batch element (float bits, order-independent max; a NaN
//      counts as +inf);
//   2. warp_bwd_scatter: each contribution wt * g scaled by 2^k_b (exact) and rounded to an
//      integer, k_b such that any source pixel's total (<= HW max|g|: the bilinear weights of
//      one reference pixel sum to <= 1) stays below 2^61; quantum 2^-k_b ~ HW max|g| 2^-62;
//   3. warp_bwd_fold: grad_src += (float)(sum 2^-k_b), one rounding.
// A batch element whose grad_out holds a NaN or an infinity has no fixed-point scale: its
// contributions go to grad_src as fp32 atomics, which carry the NaN / infinity to exactly the
// source pixels grid_sample's backward carries them to, and leave the others finite (not
// bit-reproducible, like the reference's own scatter); the fold skips it.
// Batch elements are processed 64 at a time.  Workspace: 64 exponents' source words (256 B) +
// [min(B, 64)][C][HW] int64 accumulators (zeroed here per chunk of batch elements).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) warp_bwd_max_kernel(const float* __restrict__ gout, size_t n_per_b,
                                                           unsigned* __restrict__ gmax) {
  const int b = blockIdx.y;
  const float* g = gout + (size_t)b * n_per_b;
  float m = 0.f;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n_per_b; i += (size_t)gridDim.x * 256) {
    const float v = fabsf(g[i]);
    m = (v > m || v != v) ? (v != v ? INFINITY : v) : m;
  }
  const int w = wave_reduce_i32(__float_as_int(m), 0, [](int x, int y) { return x > y ? x : y; });
  if ((threadIdx.x & 63) == 0 && (unsigned)w > __hip_atomic_load(gmax + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(gmax + b, (unsigned)w);
}

// the fixed-point exponent of a batch element; false: its grad_out is not finite
__device__ __forceinline__ bool warp_bwd_exp(unsigned maxbits, int HW, int& k) {
  const float mx = __uint_as_float(maxbits);
  k = 0;
  if (!(mx <= FLT_MAX)) return false;
  const double tot = (double)mx * (double)HW;
  if (!(tot > 0.0)) return true;
  // (the clamp is wider than any finite fp32 grad_out needs, |kk| <= ~230 down to subnormal
  // maxima: a tighter one, +-120 until the range tests, left a gradient of 2^-96 only ~40 of
  // the sum's 61 bits below its bound and cost dL/dsrc 5e-5 of its norm)
  const int kk = 61 - ilogb(tot) - 1;
  k = kk > kFixedExpMax ? kFixedExpMax : (kk < -kFixedExpMax ? -kFixedExpMax : kk);
  return true;
}

__global__ void __launch_bounds__(256) homo_warp_bwd_kernel(const float* __restrict__ gout,
                                                            const float* __restrict__ rel,
                                                            const float* __restrict__ depth,
                                                            const unsigned* __restrict__ gmax,
                                                            int C, int H, int W,
                                                            unsigned long long* __restrict__ acc,
                                                            float* __restrict__ gsrc) {
  const int b = blockIdx.y;
  const int HW = H * W;
  const float* m = rel + 12 * b;
  const float dep = depth[b];
  int k;
  const bool fixed = warp_bwd_exp(gmax[b], HW, k);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    float ix, iy;
    sample_pos(m, dep, (float)(p % W), (float)(p / W), H, W, ix, iy);
    const Taps t = make_taps(ix, iy, H, W);
    const float* g = gout + (size_t)b * C * HW + p;
    unsigned long long* s = acc + (size_t)b * C * HW;
    float* gs = gsrc + (size_t)b * C * HW;
    for (int c = 0; c < C; ++c) {
      const float gv = g[(size_t)c * HW];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (t.ok[q]) {
          if (fixed) {
            const long long f = (long long)rint(ldexp((double)(t.wt[q] * gv), k));
            if (f != 0) atomicAdd(s + (size_t)c * HW + t.idx[q], (unsigned long long)f);
          } else {
            atomicAdd(gs + (size_t)c * HW + t.idx[q], t.wt[q] * gv);
          }
        }
    }
  }
}

__global__ void __launch_bounds__(256) warp_bwd_fold_kernel(const unsigned long long* __restrict__ acc,
                                                            const unsigned* __restrict__ gmax, size_t n_per_b,
                                                            int HW, float* __restrict__ gsrc) {
  const int b = blockIdx.y;
  int k;
  if (!warp_bwd_exp(gmax[b], HW, k)) return;   // non-finite grad_out: scattered in fp32
  const unsigned long long* a = acc + (size_t)b * n_per_b;
  float* o = gsrc + (size_t)b * n_per_b;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n_per_b; i += (size_t)gridDim.x * 256) {
    const long long q = (long long)a[i];
    if (q != 0) o[i] += (float)ldexp((double)q, -k);
  }
}

constexpr int kWarpBwdChunk = 64;   // batch elements per pass (the 256-B exponent header)

static size_t homo_warp_bwd_workspace_bytes(int B, int C, int H, int W) {
  return 256 + (size_t)std::min(B, kWarpBwdChunk) * C * H * W * 8;
}

static hipError_t launch_homo_warp_bwd(const float* gout, const float* rel, const float* depth, int B,
                                       int C, int H, int W, float* gsrc, void* workspace, hipStream_t s) {
  const int HW = H * W;
  const size_t nb = (size_t)C * HW;
  unsigned* gmax = static_cast<unsigned*>(workspace);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + 256);
  ProfScope ps(s, K_WARP);
  hipError_t e = hipSuccess;
  for (int b0 = 0; b0 < B; b0 += kWarpBwdChunk) {
    const int nbt = std::min(B - b0, kWarpBwdChunk);
    if ((e = hipMemsetAsync(workspace, 0, homo_warp_bwd_workspace_bytes(nbt, C, H, W), s)) != hipSuccess)
      return e;
    const float* go = gout + (size_t)b0 * nb;
    float* gsb = gsrc + (size_t)b0 * nb;
    const unsigned gb = (unsigned)std::min<size_t>((nb + 255) / 256, 1024);
    hipLaunchKernelGGL(warp_bwd_max_kernel, dim3(gb, nbt), dim3(256), 0, s, go, nb, gmax);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    dim3 grid((unsigned)std::min((HW + 255) / 256, 4096), (unsigned)nbt);
    hipLaunchKernelGGL(homo_warp_bwd_kernel, grid, dim3(256), 0, s, go, rel + 12 * (size_t)b0, depth + b0,
                       gmax, C, H, W, acc, gsb);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(warp_bwd_fold_kernel, dim3(gb, nbt), dim3(256), 0, s, acc, gmax, nb, HW, gsb);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return e;
}

}  // namespace aarmvs

using namespace aarmvs;

extern "C" {

int aarmvs_homo_warp(const float* src_fea, const float* rel_proj, const float* depth, int B,
                     int C, int H, int W, float* out, hipStream_t stream) {
  if (!src_fea || !rel_proj || !depth || !out) return fail(AARMVS_ERR_INVALID, "homo_warp: null pointer");
  if (B < 1 || C < 1 || H < 2 || W < 2)
    return fail(AARMVS_ERR_INVALID, "homo_warp: need B>=1, C>=1, H>=2, W>=2");
  return launched(launch_homo_warp(src_fea, rel_proj, depth, B, C, H, W, out, stream), "homo_warp");
}

size_t aarmvs_homo_warp_backward_workspace_bytes(int B, int C, int H, int W) {
  if (B < 1 || C < 1 || H < 2 || W < 2) return 0;
  return homo_warp_bwd_workspace_bytes(B, C, H, W);
}

int aarmvs_homo_warp_backward(const float* grad_out, const float* rel_proj, const float* depth,
                              int B, int C, int H, int W, float* grad_src, void* workspace,
                              hipStream_t stream) {
  if (!grad_out || !rel_proj || !depth || !grad_src || !workspace)
    return fail(AARMVS_ERR_INVALID, "homo_warp_backward: null pointer");
  if (B < 1 || C < 1 || H < 2 || W < 2)
    return fail(AARMVS_ERR_INVALID, "homo_warp_backward: need B>=1, C>=1, H>=2, W>=2");
  return launched(launch_homo_warp_bwd(grad_out, rel_proj, depth, B, C, H, W, grad_src, workspace, stream),
                  "homo_warp_backward");
}

}  // extern "C"
