// The training loss from the cost volume (mvsnet_cls_loss of softmax(cost), drmvsnet.py:343-361
// restated without the probability, one-hot and log volumes) and the masked depth metrics of
// the per-epoch test pass (utils.py:150-175).  All kernels stream from HBM with no reuse: one
// thread per (b, pixel), coalesced over pixels, kUnroll planes' loads in flight, as
// softmax_depth_kernel.  Every sum is a fixed-order fp64 reduction (per-block partials, then one
// block that adds them in index order): no atomics, so the results are bit-identical run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "aarmvs_internal.h"

namespace aarmvs {

// The scratch holds [B][cls_loss_blocks(HW)][kClsPartials] fp64 per-block partials (the loss
// uses two of the slots, the metrics 2 + the thresholds); lse is [2][B][HW] (an fp32 pair).
constexpr int kClsPartials = 2 + AARMVS_MAX_THRESHOLDS;

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 8;

// Sum of v over the block's threads in a fixed order (xor butterfly inside each wave, then the
// waves in index order); the result is valid on thread 0.  N values at once share the barriers.
template <int N>
__device__ inline void block_sum(double (&v)[N], double* lds /* [kThreads / 64][N] */) {
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) lds[wave * N + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double s = lds[k];
      for (int w = 1; w < kThreads / 64; ++w) s += lds[w * N + k];
      v[k] = s;
    }
  }
}

// cost [B][D][HW], depth_gt / mask [B][HW], dvals [B][D].  Per pixel, in one pass over D: the
// online softmax state (running max m, rescaled sum s, one exp per element), the first arg-max
// of the cost (strict >), the first arg-min of |depth_value - depth_gt| (strict <, the
// reference's fp32 subtraction and abs).  gt = (int) rintf(mask * (float) argmin) is the
// reference's index rule (torch.round: half to even), clamped to [0, D - 1] so that a mask
// outside [0, 1] cannot index outside the volume (the reference's scatter_ raises there).
// ce = lse - cost[gt] with lse = m + log(s); lse is kept as an unevaluated fp32 pair (hi + lo)
// so that the backward's exp(cost - lse) is as accurate as a softmax with the max subtracted.
// lse is [2][B][HW] (hi plane, lo plane).  part [B][gridDim.x][kClsPartials]: this block's fp64
// sums of mask * ce and of mask.
__global__ void __launch_bounds__(kThreads)
cls_loss_fwd_kernel(const float* __restrict__ cost, const float* __restrict__ depth_gt,
                    const float* __restrict__ mask, const float* __restrict__ dvals, int D, int HW,
                    float* __restrict__ wta_depth, float* __restrict__ max_prob,
                    float* __restrict__ lse, int* __restrict__ gt_out, double* __restrict__ part) {
  __shared__ double lds[(kThreads / 64) * 2];
  const int b = blockIdx.y;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  const float* dv = dvals + (size_t)b * D;
  double acc[2] = {0.0, 0.0};
  if (p < HW) {
    const size_t q = (size_t)b * HW + p;
    const float* c = cost + (size_t)b * D * HW + p;
    const float gtd = depth_gt[q], mk = mask[q];
    float m = -INFINITY, s = 0.f, best = INFINITY;
    int amax = 0, amin = 0;
    auto add = [&](float v, int d) {
      const float dx = v - m;
      const float e = expf(-fabsf(dx));
      if (dx > 0.f) {   // also the first plane (m = -inf): a strictly greater cost
        s = s * e + 1.0f;
        m = v;
        amax = d;
      } else {
        s += e;
      }
      const float a = fabsf(dv[d] - gtd);
      if (a < best) {
        best = a;
        amin = d;
      }
    };
    int d = 0;
    for (; d + kUnroll <= D; d += kUnroll) {
      float v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = c[(size_t)(d + u) * HW];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) add(v[u], d + u);
    }
    for (; d < D; ++d) add(c[(size_t)d * HW], d);
    const float r = rintf(mk * (float)amin);
    const int gt = (int)fminf(fmaxf(r, 0.f), (float)(D - 1));   // NaN -> 0
    const float cg = c[(size_t)gt * HW];
    const double l = (double)m + (double)logf(s);
    const float hi = (float)l;
    lse[q] = hi;
    lse[(size_t)gridDim.y * HW + q] = (float)(l - (double)hi);
    gt_out[q] = gt;
    wta_depth[q] = dv[amax];
    if (max_prob) max_prob[q] = 1.0f / s;
    acc[0] = (double)mk * (l - (double)cg);
    acc[1] = (double)mk;
  }
  block_sum(acc, lds);
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)b * gridDim.x + blockIdx.x) * kClsPartials;
    o[0] = acc[0];
    o[1] = acc[1];
  }
}

// One block: per batch element the partials in index order (thread t takes t, t + 256, ...,
// then the block's fixed-order sum), loss = mean_b(sum mask ce / (sum mask + 1e-6)) and
// coef[b] = 1 / ((sum mask + 1e-6) B).
__global__ void __launch_bounds__(kThreads)
cls_loss_reduce_kernel(const double* __restrict__ part, int B, int nblk, float* __restrict__ loss,
                       float* __restrict__ coef) {
  __shared__ double lds[(kThreads / 64) * 2];
  double total = 0.0;
  for (int b = 0; b < B; ++b) {
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += kThreads) {
      const double* o = part + ((size_t)b * nblk + i) * kClsPartials;
      acc[0] += o[0];
      acc[1] += o[1];
    }
    block_sum(acc, lds);
    if (threadIdx.x == 0) {
      const double valid = acc[1] + 1e-6;
      total += acc[0] / valid;
      coef[b] = (float)(1.0 / (valid * (double)B));
    }
    __syncthreads();   // lds is reused by the next element
  }
  if (threadIdx.x == 0) *loss = (float)(total / (double)B);
}

// grad_cost[b,d,p] = g coef[b] mask[b,p] (exp(cost - lse) - [d == gt]); g is read from the
// device.  A pixel whose factor is zero (mask 0) writes zeros without reading the cost.
__global__ void __launch_bounds__(kThreads)
cls_loss_bwd_kernel(const float* __restrict__ cost, const float* __restrict__ lse,
                    const int* __restrict__ gt_in, const float* __restrict__ mask,
                    const float* __restrict__ coef, const float* __restrict__ g, int D, int HW,
                    float* __restrict__ grad_cost) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= HW) return;
  const size_t q = (size_t)b * HW + p;
  const float* c = cost + (size_t)b * D * HW + p;
  float* o = grad_cost + (size_t)b * D * HW + p;
  const float f = (g[0] * coef[b]) * mask[q];
  if (f == 0.f) {
    for (int d = 0; d < D; ++d) o[(size_t)d * HW] = 0.f;
    return;
  }
  const float hi = lse[q], lo = lse[(size_t)gridDim.y * HW + q];
  const int gt = gt_in[q];
  int d = 0;
  for (; d + kUnroll <= D; d += kUnroll) {
    float v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) v[u] = c[(size_t)(d + u) * HW];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      o[(size_t)(d + u) * HW] = f * (expf((v[u] - hi) - lo) - (d + u == gt ? 1.f : 0.f));
  }
  for (; d < D; ++d)
    o[(size_t)d * HW] = f * (expf((c[(size_t)d * HW] - hi) - lo) - (d == gt ? 1.f : 0.f));
}

struct Thresholds {
  float v[AARMVS_MAX_THRESHOLDS];
};

// est / gt / mask [B][HW].  Over the pixels with mask > 0.5: their number, the sum of
// |est - gt| (the reference's fp32 difference) and per threshold the number with
// |est - gt| > thr, as this block's fp64 partials part [B][gridDim.x][kClsPartials].
__global__ void __launch_bounds__(kThreads)
depth_metrics_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                     const float* __restrict__ mask, int HW, Thresholds thr, int nthr,
                     double* __restrict__ part) {
  __shared__ double lds[(kThreads / 64) * kClsPartials];
  const int b = blockIdx.y;
  const int p = blockIdx.x * kThreads + threadIdx.x;
  double acc[kClsPartials];
#pragma unroll
  for (int k = 0; k < kClsPartials; ++k) acc[k] = 0.0;
  if (p < HW) {
    const size_t q = (size_t)b * HW + p;
    if (mask[q] > 0.5f) {
      const float e = fabsf(est[q] - gt[q]);
      acc[0] = 1.0;
      acc[1] = (double)e;
#pragma unroll
      for (int k = 0; k < AARMVS_MAX_THRESHOLDS; ++k)
        if (k < nthr && e > thr.v[k]) acc[2 + k] = 1.0;
    }
  }
  block_sum(acc, lds);
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)b * gridDim.x + blockIdx.x) * kClsPartials;
#pragma unroll
    for (int k = 0; k < kClsPartials; ++k) o[k] = acc[k];
  }
}

// One block: out[0] = mean_b(sum |est - gt| / n_b), out[1 + k] = mean_b(count_k / n_b); an
// element with no valid pixel gives 0 / 0 = NaN, as torch.mean of an empty tensor.
__global__ void __launch_bounds__(kThreads)
depth_metrics_reduce_kernel(const double* __restrict__ part, int B, int nblk, int nthr,
                            double* __restrict__ out) {
  __shared__ double lds[(kThreads / 64) * kClsPartials];
  double total[1 + AARMVS_MAX_THRESHOLDS];
#pragma unroll
  for (int k = 0; k < 1 + AARMVS_MAX_THRESHOLDS; ++k) total[k] = 0.0;
  for (int b = 0; b < B; ++b) {
    double acc[kClsPartials];
#pragma unroll
    for (int k = 0; k < kClsPartials; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < nblk; i += kThreads) {
      const double* o = part + ((size_t)b * nblk + i) * kClsPartials;
#pragma unroll
      for (int k = 0; k < kClsPartials; ++k) acc[k] += o[k];
    }
    block_sum(acc, lds);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 1 + AARMVS_MAX_THRESHOLDS; ++k) total[k] += acc[1 + k] / acc[0];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 1 + AARMVS_MAX_THRESHOLDS; ++k)
      if (k <= nthr) out[k] = total[k] / (double)B;
  }
}

}  // namespace

static int cls_loss_blocks(int HW) { return (HW + kThreads - 1) / kThreads; }

static hipError_t launch_cls_loss_fwd(const float* cost, const float* depth_gt, const float* mask,
                                      const float* dvals, int B, int D, int HW, float* loss,
                                      float* wta_depth, float* max_prob, float* lse, int* gt, float* coef,
                                      void* scratch, hipStream_t s) {
  const int nblk = cls_loss_blocks(HW);
  double* part = static_cast<double*>(scratch);
  {
    ProfScope ps(s, K_CLS_LOSS_FWD);
    hipLaunchKernelGGL(cls_loss_fwd_kernel, dim3(nblk, B), dim3(kThreads), 0, s, cost, depth_gt, mask,
                       dvals, D, HW, wta_depth, max_prob, lse, gt, part);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  ProfScope ps(s, K_CLS_LOSS_REDUCE);
  hipLaunchKernelGGL(cls_loss_reduce_kernel, dim3(1), dim3(kThreads), 0, s, part, B, nblk, loss, coef);
  return hipGetLastError();
}

static hipError_t launch_cls_loss_bwd(const float* cost, const float* lse, const int* gt, const float* mask,
                                      const float* coef, const float* g, int B, int D, int HW,
                                      float* grad_cost, hipStream_t s) {
  ProfScope ps(s, K_CLS_LOSS_BWD);
  hipLaunchKernelGGL(cls_loss_bwd_kernel, dim3(cls_loss_blocks(HW), B), dim3(kThreads), 0, s, cost,
                     lse, gt, mask, coef, g, D, HW, grad_cost);
  return hipGetLastError();
}

static hipError_t launch_depth_metrics(const float* est, const float* gt, const float* mask, int B, int HW,
                                       const float* thresholds, int nthr, double* out, void* scratch,
                                       hipStream_t s) {
  const int nblk = cls_loss_blocks(HW);
  double* part = static_cast<double*>(scratch);
  Thresholds thr{};
  for (int k = 0; k < nthr; ++k) thr.v[k] = thresholds[k];
  ProfScope ps(s, K_DEPTH_METRICS);
  hipLaunchKernelGGL(depth_metrics_kernel, dim3(nblk, B), dim3(kThreads), 0, s, est, gt, mask, HW,
                     thr, nthr, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(depth_metrics_reduce_kernel, dim3(1), dim3(kThreads), 0, s, part, B, nblk, nthr,
                     out);
  return hipGetLastError();
}

}  // namespace aarmvs

using namespace aarmvs;

extern "C" {

// B rides in gridDim.y; the pixel index of a block's last thread must fit an int
static int cls_check(const char* who, int B, int HW) {
  if (B < 1 || HW < 1) return fail(AARMVS_ERR_INVALID, std::string(who) + ": need B, HW >= 1");
  if (B > 65535 || HW > 0x7fffffff - 256)
    return fail(AARMVS_ERR_INVALID, std::string(who) + ": need B <= 65535 and HW < 2^31 - 256");
  return AARMVS_OK;
}

size_t aarmvs_cls_loss_scratch_bytes(int B, int HW) {
  if (cls_check("cls_loss_scratch_bytes", B, HW)) return 0;
  return (size_t)B * cls_loss_blocks(HW) * kClsPartials * sizeof(double);
}

int aarmvs_cls_loss(const float* cost, const float* depth_gt, const float* mask,
                    const float* depth_values, int B, int D, int HW, float* loss, float* wta_depth,
                    float* max_prob, float* lse, int* gt_index, float* coef, void* scratch,
                    hipStream_t stream) {
  if (!cost || !depth_gt || !mask || !depth_values || !loss || !wta_depth || !lse || !gt_index ||
      !coef || !scratch)
    return fail(AARMVS_ERR_INVALID, "cls_loss: null pointer argument");
  if (int rc = cls_check("cls_loss", B, HW)) return rc;
  if (D < 1) return fail(AARMVS_ERR_INVALID, "cls_loss: need D >= 1");
  return launched(launch_cls_loss_fwd(cost, depth_gt, mask, depth_values, B, D, HW, loss, wta_depth,
                                      max_prob, lse, gt_index, coef, scratch, stream),
                  "cls_loss");
}

int aarmvs_cls_loss_backward(const float* cost, const float* lse, const int* gt_index,
                             const float* mask, const float* coef, const float* grad_loss, int B,
                             int D, int HW, float* grad_cost, hipStream_t stream) {
  if (!cost || !lse || !gt_index || !mask || !coef || !grad_loss || !grad_cost)
    return fail(AARMVS_ERR_INVALID, "cls_loss_backward: null pointer argument");
  if (int rc = cls_check("cls_loss_backward", B, HW)) return rc;
  if (D < 1) return fail(AARMVS_ERR_INVALID, "cls_loss_backward: need D >= 1");
  return launched(launch_cls_loss_bwd(cost, lse, gt_index, mask, coef, grad_loss, B, D, HW, grad_cost, stream),
                  "cls_loss_backward");
}

int aarmvs_depth_metrics(const float* depth_est, const float* depth_gt, const float* mask, int B,
                         int HW, const float* thresholds, int n_thresholds, double* out,
                         void* scratch, hipStream_t stream) {
  if (!depth_est || !depth_gt || !mask || !out || !scratch || (n_thresholds > 0 && !thresholds))
    return fail(AARMVS_ERR_INVALID, "depth_metrics: null pointer argument");
  if (int rc = cls_check("depth_metrics", B, HW)) return rc;
  if (n_thresholds < 0 || n_thresholds > AARMVS_MAX_THRESHOLDS)
    return fail(AARMVS_ERR_INVALID, "depth_metrics: at most 8 thresholds");
  return launched(launch_depth_metrics(depth_est, depth_gt, mask, B, HW, thresholds, n_thresholds, out,
                                       scratch, stream),
                  "depth_metrics");
}

}  // extern "C"
