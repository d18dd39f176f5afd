// ===========================================================================
// Backward of the cost-slice stage (the BPTT's drmvsnet.py:307-319 part): from dL/dx of a
// group of planes to the omega.* parameter gradients and dL/d(reference, source features).
//   x = -(1/nsrc) sum_v (1 + w_v) sq_v,  sq_v = (warp_v - ref)^2,  w_v = omega(sq_v)
//   dL/dsq_v = -(1 + w_v)/nsrc dL/dx + conv3x3^T(dL/dt1_v);  dL/dw_v = -(1/nsrc) sum_c dL/dx sq_v
//   omega chain backward (sigmoid, 1x1 conv, ReLU, ResnetBlockGn with three GroupNorm(1,4)
//   backwards, each needing a grid-wide sum per (plane, sample, view))
//   dL/dwarp_v = 2 (warp_v - ref) dL/dsq_v;  dL/dref = -sum_v dL/dwarp_v;
//   dL/dsrc_v = bilinear scatter of dL/dwarp_v (module.py:36: grid_sample's backward).
// The forward's t1 and GroupNorm statistics come from the training record (the forward copies
// them there per group); every pixel's warp, sq and omega chain is recomputed with the
// forward's own arithmetic (same helpers, contraction off), so the ReLU masks are the forward's.
// Stages per group: cbw_chain<1> (dL/dw from the warp, dL/do; GN3 sums), <2> (GN2 sums),
// <3> (GN1 sums), <4> (dL/dt1), each with a fixed-order reduce; cbw_feat (dL/dsq, the
// feature gradients, the conv3x3 weight gradient).  Source gradients are scattered into an
// LDS box per (tile, view) over the group's planes and flushed with global atomics.
// ===========================================================================

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstring>

#include "cost_device.h"

namespace aarmvs {

// omega chain of one (pixel, view) with its intermediates (omega_weight's operations)
struct OmegaChain {
  float t[4], v1[4], aa[4], t2[4], v2[4], bb[4], t3[4], g3[4], s3[4], w;
};
__device__ __forceinline__ void omega_chain(const float4 q, const GnStat* gs, const OmegaP& o,
                                            OmegaChain& c) {
  c.t[0] = q.x;
  c.t[1] = q.y;
  c.t[2] = q.z;
  c.t[3] = q.w;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float sc = gs[0].rstd * o.g0w[i];
    const float sh = o.g0b[i] - gs[0].mean * sc;
    c.v1[i] = c.t[i] * sc + sh;
    c.aa[i] = fmaxf(c.v1[i], 0.0f);
  }
  conv1x1_4(c.aa, o.w1, o.b1, c.t2);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float sc = gs[1].rstd * o.g1w[i];
    const float sh = o.g1b[i] - gs[1].mean * sc;
    c.v2[i] = c.t2[i] * sc + sh;
    c.bb[i] = fmaxf(c.v2[i], 0.0f);
  }
  conv1x1_4(c.bb, o.w2, o.b2, c.t3);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float sc = gs[2].rstd * o.g2w[i];
    const float sh = o.g2b[i] - gs[2].mean * sc;
    c.g3[i] = c.t3[i] * sc + sh;
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c.s3[i] = c.g3[i] + c.aa[i];
    s = fmaf(o.wo[i], fmaxf(c.s3[i], 0.0f), s);
  }
  c.w = sigmoidf_(s + o.bo);
}

struct CbwArgs {
  PipeArgs p;            // forward pipeline arguments (c8 features, rel, depths, params, t1, stats)
  const float* gx;       // [n][B][HW][32] dL/dx of the group's planes
  float* go;             // [n][B][nsrc][HW] dL/do (stage 1 out, later in)
  float* wo;             // [n][B][nsrc][HW] the omega weights w (stage 1 out, for cbw_feat)
  float4* gt1;           // [n][B][nsrc][HW] dL/dt1 (stage 4 out)
  const double* gsum;    // [n][B][nsrc][3][2] GroupNorm backward sums (stage 1: GN3, 2: GN2, 3: GN1)
  double* part;          // [n][B][nsrc][pblk][32] per-block partial sums
  unsigned* gmax;        // float bits: [0] max |dL/dx| (stage 1), [1] max |dL/dt1| (stage 4)
  int d0, pblk;
};

// max |v| of a wave folded into *dst (float bits: non-negative floats order as unsigned; an
// order-independent, hence deterministic, reduction)
__device__ __forceinline__ void wave_absmax_bits(float m, unsigned* dst) {
  const int b = wave_reduce_i32(__float_as_int(m != m ? INFINITY : m), 0,
                                [](int x, int y) { return x > y ? x : y; });
  if ((threadIdx.x & 63) == 0 && (unsigned)b > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(dst, (unsigned)b);
}

// columns of each stage's partial rows: 0, 1 = the GroupNorm sums of the stage's statistic;
// then parameter-gradient sums (cbw_param_cols)
template <int STAGE>
__global__ void __launch_bounds__(256) cbw_chain_kernel(CbwArgs a, const float* __restrict__ P,
                                                        const float* __restrict__ Rel) {
  constexpr int NCOL = STAGE == 1 ? 15 : STAGE == 4 ? 4 : 30;
  __shared__ double red[NCOL * 4];
  __shared__ GnStat gs[3];
  __shared__ float gm[3][2];   // per statistic: mean(g_xhat), mean(g_xhat xhat)
  const PipeArgs& pa = a.p;
  const int v = blockIdx.y, bk = blockIdx.z, b = bk % pa.B, k = bk / pa.B;
  const int H = pa.H, W = pa.W, HW = H * W, nsrc = pa.nsrc;
  const size_t kbv = ((size_t)k * pa.B + b) * nsrc + v;
  if (threadIdx.x < 3)
    gs[threadIdx.x] = stat_read(pa.st_prev + k * pa.st_kstride + st_index(b, v, threadIdx.x, nsrc), 4.0 * HW);
  if (threadIdx.x >= 32 && threadIdx.x < 38) {
    const int i = threadIdx.x - 32;   // statistic 2 - (i >> 1)... (GN3 = stat 2, GN2 = 1, GN1 = 0)
    const int st = i >> 1;
    gm[st][i & 1] = (float)(a.gsum[kbv * 6 + 2 * st + (i & 1)] / (4.0 * HW));
  }
  __syncthreads();
  OmegaP o;
  load_omega(pa, P, o);
  double s[NCOL];   // fp64: the parameter gradients are long cancelling sums
#pragma unroll
  for (int i = 0; i < NCOL; ++i) s[i] = 0.0;
  const float* m = Rel + 12 * (v * pa.B + b);
  const float dep = pa.dvals[b * pa.D + a.d0 + k];
  const uint32_t fbytes = (uint32_t)((size_t)kC * HW * 4);
  const __amdgpu_buffer_rsrc_t rref = uniform_rsrc(pa.ref + (size_t)b * kC * HW, fbytes);
  const __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(pa.src[v] + (size_t)b * kC * HW, fbytes);
  const float4* t1p = pa.t1_prev + k * pa.t1_kstride + ((size_t)b * nsrc + v) * HW;
  float* gop = a.go + kbv * HW;
  float amax = 0.f;   // stage 1: max |dL/dx|, stage 4: max |dL/dt1| (the dL/dsrc fixed-point scale)
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    OmegaChain c;
    omega_chain(t1p[p], gs, o, c);
    float g_o;
    if constexpr (STAGE == 1) {
      // dL/dw = -(1/nsrc) sum_c dL/dx sq (the warp and sq recomputed as cost_x does)
      const int x = p % W, y = p / W;
      const TapF tf = tap_f(m, dep, x, y, H, W);
      const Box none{0, 0, 0, 0};
      const TapP t = tap_p(tf, true, H, W, false, none, fbytes / 32u);
      const float* gxp = a.gx + (((size_t)k * pa.B + b) * HW + p) * kC;
      float dw = 0.f;
#pragma unroll
      for (int sl = 0; sl < 8; ++sl) {
        const float4 g = bil4(ld_c8(rsrc, t.pix[0], sl, HW), ld_c8(rsrc, t.pix[1], sl, HW),
                              ld_c8(rsrc, t.pix[2], sl, HW), ld_c8(rsrc, t.pix[3], sl, HW), t);
        const float4 sq = sqdiff4(g, ld_c8(rref, (uint32_t)p, sl, HW));
        const float4 gg = *reinterpret_cast<const float4*>(gxp + 4 * sl);
        dw += gg.x * sq.x + gg.y * sq.y + gg.z * sq.z + gg.w * sq.w;
        amax = fmaxf(amax, fmaxf(fmaxf(fabsf(gg.x), fabsf(gg.y)), fmaxf(fabsf(gg.z), fabsf(gg.w))));
      }
      dw = -dw / (float)nsrc;
      g_o = dw * c.w * (1.0f - c.w);
      gop[p] = g_o;
      a.wo[kbv * HW + p] = c.w;
    } else {
      g_o = gop[p];
    }
    float g_r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) g_r[i] = c.s3[i] > 0.f ? o.wo[i] * g_o : 0.f;
    // GN3 (statistic 2): y = g3 = gamma xhat + beta, dL/dy = g_r
    float xh3[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xh3[i] = (c.t3[i] - gs[2].mean) * gs[2].rstd;
    if constexpr (STAGE == 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float gx3 = g_r[i] * o.g2w[i];
        s[0] += gx3;
        s[1] += gx3 * xh3[i];
        s[2 + i] += g_o * fmaxf(c.s3[i], 0.0f);   // Wo
        s[7 + i] += g_r[i] * xh3[i];               // gamma3
        s[11 + i] += g_r[i];                       // beta3
      }
      s[6] += g_o;                                 // bo
      continue;
    }
    float g_t3[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) g_t3[i] = gs[2].rstd * (g_r[i] * o.g2w[i] - gm[2][0] - xh3[i] * gm[2][1]);
    // t3 = W2 bb + b2
    float g_n2[4], xh2[4];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      float ga = 0.f;
#pragma unroll
      for (int co = 0; co < 4; ++co) ga = fmaf(o.w2[co * 4 + ci], g_t3[co], ga);
      g_n2[ci] = c.v2[ci] > 0.f ? ga : 0.f;
      xh2[ci] = (c.t2[ci] - gs[1].mean) * gs[1].rstd;
    }
    if constexpr (STAGE == 2) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float gx2 = g_n2[i] * o.g1w[i];
        s[0] += gx2;
        s[1] += gx2 * xh2[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[2 + i * 4 + j] += g_t3[i] * c.bb[j];   // W2[i][j]
        s[18 + i] += g_t3[i];                                              // b2
        s[22 + i] += g_n2[i] * xh2[i];                                     // gamma2
        s[26 + i] += g_n2[i];                                              // beta2
      }
      continue;
    }
    float g_t2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) g_t2[i] = gs[1].rstd * (g_n2[i] * o.g1w[i] - gm[1][0] - xh2[i] * gm[1][1]);
    // t2 = W1 aa + b1; aa also feeds the residual (r = relu(g3 + aa))
    float g_n1[4], xh1[4];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      float ga = g_r[ci];
#pragma unroll
      for (int co = 0; co < 4; ++co) ga = fmaf(o.w1[co * 4 + ci], g_t2[co], ga);
      g_n1[ci] = c.v1[ci] > 0.f ? ga : 0.f;
      xh1[ci] = (c.t[ci] - gs[0].mean) * gs[0].rstd;
    }
    if constexpr (STAGE == 3) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float gx1 = g_n1[i] * o.g0w[i];
        s[0] += gx1;
        s[1] += gx1 * xh1[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[2 + i * 4 + j] += g_t2[i] * c.aa[j];   // W1[i][j]
        s[18 + i] += g_t2[i];                                              // b1
        s[22 + i] += g_n1[i] * xh1[i];                                     // gamma1
        s[26 + i] += g_n1[i];                                              // beta1
      }
      continue;
    }
    float g_t1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      g_t1[i] = gs[0].rstd * (g_n1[i] * o.g0w[i] - gm[0][0] - xh1[i] * gm[0][1]);
      s[i] += g_t1[i];   // b0
    }
    a.gt1[kbv * HW + p] = make_float4(g_t1[0], g_t1[1], g_t1[2], g_t1[3]);
    amax = fmaxf(amax, fmaxf(fmaxf(fabsf(g_t1[0]), fabsf(g_t1[1])), fmaxf(fabsf(g_t1[2]), fabsf(g_t1[3]))));
  }
  if constexpr (STAGE == 1 || STAGE == 4) wave_absmax_bits(amax, a.gmax + (STAGE == 1 ? 0 : 1));
  block_sum_d_store<NCOL>(s, red, a.part + (kbv * a.pblk + blockIdx.x) * 32);
}

// GroupNorm-backward sums per (plane, b, v): columns 0, 1 of the stage's partial rows
__global__ void cbw_gsum_kernel(const double* __restrict__ part, int pblk, double* __restrict__ gsum,
                                int st) {
  const size_t kbv = blockIdx.x;
  const int c = threadIdx.x;
  if (c >= 2) return;
  double s = 0.0;
  for (int i = 0; i < pblk; ++i) s += part[(kbv * pblk + i) * 32 + c];
  gsum[kbv * 6 + 2 * st + c] = s;
}

// parameter columns -> gacc: one block per column, strided per-thread sums then a fixed tree
struct CbwCols {
  int c0, ncol;
  int off[30];   // gacc index of column c0 + j
};
__global__ void __launch_bounds__(256) cbw_param_kernel(const double* __restrict__ part, int nrow,
                                                        CbwCols cols, double* __restrict__ gacc) {
  __shared__ double red[256];
  const int t = threadIdx.x, j = blockIdx.x;
  double s = 0.0;
  for (int r = t; r < nrow; r += 256) s += part[(size_t)r * 32 + cols.c0 + j];
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) gacc[cols.off[j]] += red[0];
}

// dL/dsrc in fixed point: the scatter of grid_sample's backward adds contributions from many
// blocks into one source pixel, and fp32 atomics would make the sum depend on their order.  Each
// contribution (an fp32 value, or a block's fp32 register sum over its own gathers, formed in a
// fixed order) is scaled by 2^k (exact) and rounded to a 64-bit integer; integer atomics are
// associative, so the group's sums are bit-reproducible.  k is chosen per group from a bound on
// any source pixel's total (cbw_scale_kernel), so nothing overflows and the fixed-point quantum
// is ~2^-40 of that bound (far below float32's resolution of the values).
__device__ __forceinline__ unsigned long long to_fixed(float v, int k) {
  return (unsigned long long)(long long)rintf(ldexpf(v, k));
}

// k from the group's maxima: |dL/dwarp| = |2 (warp - ref) dL/dsq| <= 4 max|f| (2/nsrc max|dL/dx| +
// 36 max|w0| max|dL/dt1|) =: G (|warp|, |ref| <= max|f| = sqrt(xbound / 8)), every reference pixel
// and plane contributes at most G in total (bilinear weights sum to <= 1), so any source pixel's
// sum over the group is <= HW n G; 2^k HW n G <= 2^61.
__global__ void cbw_scale_kernel(const unsigned* __restrict__ gmax, const unsigned* __restrict__ xbound,
                                 const float* __restrict__ w0, int HW, int n, int nsrc, int* __restrict__ fxk) {
  __shared__ float red[64];
  float mw = 0.f;
  for (int i = threadIdx.x; i < 4 * 32 * 9; i += 64) mw = fmaxf(mw, fabsf(w0[i]));
  red[threadIdx.x] = mw;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 64; ++i) mw = fmaxf(mw, red[i]);
    const double mf = sqrt((double)__uint_as_float(*xbound) / 8.0);
    const double g = 4.0 * mf * (2.0 / nsrc * (double)__uint_as_float(gmax[0]) +
                                 36.0 * (double)mw * (double)__uint_as_float(gmax[1]));
    const double tot = g * (double)HW * (double)n;
    int k = 0;
    if (tot > 0.0 && tot < 1e300) {
      k = 61 - ilogb(tot) - 1;   // never clamped for finite fp32 maxima (warp_bwd_exp)
      k = k > kFixedExpMax ? kFixedExpMax : (k < -kFixedExpMax ? -kFixedExpMax : k);
    }
    *fxk = k;
  }
}

// gsrc8 += the group's fixed-point sums (value 2^-k), which are cleared for the next group:
// the groups are folded in their fixed (reverse plane) order
// AARMVS_COH (diagnostic builds only, tools/bwd_nondet.py): the cost-slice backward's reads of
// buffers written by earlier kernels as agent-scope atomic loads, its read-modify-writes as
// agent-scope atomic loads and stores (L2-coherent across XCDs); the library is built with 0
#ifndef AARMVS_COH
#define AARMVS_COH 0
#endif
template <typename T>
__device__ __forceinline__ T coh_ld(const T* p) {
  if constexpr (AARMVS_COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <typename T>
__device__ __forceinline__ void coh_st(T* p, T v) {
  if constexpr (AARMVS_COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
__device__ __forceinline__ float4 coh_ld4(const float* p) {
  if constexpr (AARMVS_COH) return make_float4(coh_ld(p), coh_ld(p + 1), coh_ld(p + 2), coh_ld(p + 3));
  else return *reinterpret_cast<const float4*>(p);
}
__global__ void __launch_bounds__(256) cbw_fold_kernel(unsigned long long* __restrict__ g64,
                                                       float* __restrict__ gsrc8, size_t n,
                                                       const int* __restrict__ fxk) {
  const int k = *fxk;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const long long q = (long long)coh_ld(g64 + i);
    if (q != 0) {
      coh_st(gsrc8 + i, coh_ld(gsrc8 + i) + (float)ldexp((double)q, -k));
      coh_st(g64 + i, 0ull);
    }
  }
}

// dL/dsq, the feature gradients and the conv3x3 weight gradient.  Block: a 16 x 16 tile of one
// sample, one source view and one 8-channel chunk, all planes of the group; thread = pixel.
//   dL/dsq = -(1 + w)/nsrc dL/dx + conv3x3^T(dL/dt1)   (this chunk's 8 channels)
//   dL/dwarp = 2 (warp - ref) dL/dsq;  dL/dref -= dL/dwarp (per view, summed in view order by
//   cost_bwd_end: one writer per (view, pixel, channel));
//   dL/dsrc: grid_sample's bilinear scatter of dL/dwarp, done as a gather.  The source box (the
//   bounding box of the tile's taps over the group's planes: corner positions bound them, the
//   plane homography and the position along a depth ray being monotone while z > 0) is owned
//   pixel by pixel by the block's threads, which accumulate in registers over the planes.  Per
//   plane every reference pixel files its index under the box cell of its top-left tap (one
//   integer LDS atomic for the slot); each owned source pixel then reads the cells of its four
//   possible top-left taps and adds wt[corner] * dL/dwarp of the pixels filed there.  After the
//   group the owned pixels are flushed with global atomics (neighbouring tiles' boxes overlap).
//   A cell with more than kFbSlots pixels, a tap outside the box, or a box that does not fit
//   (kFbOwn pixels per thread) uses global atomics directly.  (The LDS box of float atomics this
//   replaces took half of the kernel: 32 ds_add_f32 per pixel and plane.)
//   gW0[co][c][tap] = sum_q dL/dt1[q - off(tap)][co] sq[q][c]: thread t < 252 owns (half of the
//   chunk's channels, tap) pair t % 18 for all four co (16 sums: one float4 read of sq and one of
//   dL/dt1 per 16 FMAs) over the tile pixels q = t / 18 + 14 i; the 14 pixel subsets are summed in
//   order at the end.
constexpr int kFbT = 16, kFbOwn = 3, kFbBoxPx = kFbOwn * 256, kFbCells = 1280, kFbSlots = 2;
constexpr int kWgPairs = 18, kWgSubs = 14;
// LDS scratch of the plane loop (gather cells, filed dL/dwarp and weights), reused after the
// loop for the weight-gradient subset sums
constexpr int kFbGwOff = 0, kFbWtOff = 256 * 32, kFbCntOff = kFbWtOff + 256 * 16,
              kFbLstOff = kFbCntOff + kFbCells * 4, kFbScratch = kFbLstOff + kFbCells * kFbSlots * 2;
static_assert(kFbScratch >= kWgPairs * kWgSubs * 16 * 4, "subset sums fit the scratch");
struct CbfArgs {
  PipeArgs p;
  const float* gx;          // [n][B][HW][32]
  const float4* gt1;        // [n][B][nsrc][HW]
  const float* w;           // [n][B][nsrc][HW] omega weights (cbw_chain<1>'s)
  unsigned long long* gsrc64;   // [nsrc][B][4][HW][8] the group's dL/dsrc (c8 layout) in fixed point
  const int* fxk;           // the fixed-point exponent k: value = integer 2^-k (cbw_scale_kernel)
  float* grefv;             // [nsrc][B][32][HW] dL/dref per view (NCHW) accumulated
  float* wpart;             // [4 chunks][nsrc][B][tiles][288] conv3x3 weight-gradient partials
  int d0, n;
};

#ifndef AARMVS_CBF_MINB
#define AARMVS_CBF_MINB 2
#endif
// diagnostic builds only (tools/lib_variant.sh): 1 no weight-gradient loop, 2 no scatter, 4 no source
// gathers, 8 no box flush, 16 no conv3x3^T; the library is built with 0
#ifndef AARMVS_CBF_ABL
#define AARMVS_CBF_ABL 0
#endif
__global__ void __launch_bounds__(256, AARMVS_CBF_MINB) cbw_feat_kernel(CbfArgs a, const float* __restrict__ P,
                                                       const float* __restrict__ Rel) {
  __shared__ float4 w0q[9][8];                    // this chunk's conv3x3 weights [tap][c] (co in .xyzw)
  __shared__ float4 gts[18 * 18];                 // dL/dt1 of the haloed tile (one plane)
  __shared__ float4 sq4[256][2];                  // the tile's sq (8 channels)
  __shared__ __attribute__((aligned(16))) char fbs[kFbScratch];
  float4 (*const gwim)[2] = reinterpret_cast<float4 (*)[2]>(fbs + kFbGwOff);   // dL/dwarp (8 ch)
  float4* const wtim = reinterpret_cast<float4*>(fbs + kFbWtOff);              // bilinear weights
  int* const cnt = reinterpret_cast<int*>(fbs + kFbCntOff);   // pixels filed per top-left-tap cell
  unsigned short (*const lst)[kFbSlots] =
      reinterpret_cast<unsigned short (*)[kFbSlots]>(fbs + kFbLstOff);         // their tile indices
  float (*const wsum)[kWgSubs][16] = reinterpret_cast<float (*)[kWgSubs][16]>(fbs);   // after the loop
  __shared__ int bred[4][4];
  __shared__ int bad;
  const PipeArgs& pa = a.p;
  const int tid = threadIdx.x, b = blockIdx.z;
  // one block per (tile, view, chunk), chunk fastest, XCD-aware (xcd_tile): the 4 nsrc blocks
  // of a tile, which read the same dL/dx (and per view the same dL/dt1 halo) lines, and the
  // neighbouring tiles, which share source taps, run together on one XCD's L2
  const int seq = xcd_tile(blockIdx.x, gridDim.x);
  const int tile = seq / (4 * pa.nsrc), vc = seq - tile * (4 * pa.nsrc);
  const int v = vc >> 2, c = vc & 3;
  const int fxk = *a.fxk;
  const int H = pa.H, W = pa.W, HW = H * W, nsrc = pa.nsrc;
  const int tiles_x = (W + kFbT - 1) / kFbT;
  const int tx0 = (tile % tiles_x) * kFbT, ty0 = (tile / tiles_x) * kFbT;
  const int lx = tid & 15, ly = tid >> 4;
  const int x = tx0 + lx, y = ty0 + ly;
  const bool in = x < W && y < H;
  const int p = in ? y * W + x : 0;
  if (tid < 72) {   // raw [co][32][tap]
    const int tap = tid % 9, j = tid / 9;
    const float* w = P + pa.off_ow0 + (8 * c + j) * 9 + tap;
    w0q[tap][j] = make_float4(w[0], w[288], w[576], w[864]);
  }
  if (tid == 0) bad = 0;
  const uint32_t fbytes = (uint32_t)((size_t)kC * HW * 4);
  const __amdgpu_buffer_rsrc_t rref = uniform_rsrc(pa.ref + (size_t)b * kC * HW, fbytes);
  const __amdgpu_buffer_rsrc_t rsrc = uniform_rsrc(pa.src[v] + (size_t)b * kC * HW, fbytes);
  const float* m = Rel + 12 * (v * pa.B + b);
  const int pair = tid % kWgPairs, sub = tid / kWgPairs;   // weight-gradient role (tid < 252)
  const int pcg = pair / 9, ptap = pair % 9;
  float gref[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float wacc[16];   // [co][4 channels of half pcg]
#pragma unroll
  for (int i = 0; i < 16; ++i) wacc[i] = 0.f;
  const float4 rf0 = in ? ld_c8(rref, (uint32_t)p, 2 * c, HW) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 rf1 = in ? ld_c8(rref, (uint32_t)p, 2 * c + 1, HW) : make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  // the source box over the group's planes: tile corners x planes
  int bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
  if (tid < 4 * a.n) {
    const int cx = (tid & 1) ? min(tx0 + kFbT - 1, W - 1) : tx0;
    const int cy = (tid & 2) ? min(ty0 + kFbT - 1, H - 1) : ty0;
    const float dep = pa.dvals[b * pa.D + a.d0 + (tid >> 2)];
    const float zc = (m[8] * (float)cx + m[9] * (float)cy + m[10]) * dep + m[11];
    const TapF tf = tap_f(m, dep, cx, cy, H, W);
    if (!(zc > 0.f) || !(tf.xf == tf.xf) || !(tf.yf == tf.yf) || fabsf(tf.xf) > 1e6f ||
        fabsf(tf.yf) > 1e6f) {
      bad = 1;
    } else {
      bx0 = max(0, (int)tf.xf);
      by0 = max(0, (int)tf.yf);
      bx1 = min(W - 1, (int)tf.xf + 1);
      by1 = min(H - 1, (int)tf.yf + 1);
    }
  }
  const Box bxr = box_reduce<4>(bx0, by0, bx1, by1, bred);
  // cells: top-left tap positions x0 - 1 .. x0 + nx - 1 (and likewise in y), row stride cw
  const int cw = bxr.nx + 1;
  const bool use_box = !bad && bxr.nx > 0 && bxr.ny > 0 && bxr.nx * bxr.ny <= kFbBoxPx &&
                       cw * (bxr.ny + 1) <= kFbCells;
  if (use_box)
    for (int i = tid; i < cw * (bxr.ny + 1); i += 256) cnt[i] = 0;
  float own[kFbOwn][8];   // owned source-box pixels tid + 256 j: dL/dsrc over the group's planes
#pragma unroll
  for (int j = 0; j < kFbOwn; ++j)
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) own[j][ch] = 0.f;
  int mycell = -1;        // the cell this thread's pixel was filed under (reset next plane)
  int obase[kFbOwn];      // cell of owned pixel j's own position (its corner-0 cell), or -1
#pragma unroll
  for (int j = 0; j < kFbOwn; ++j) {
    const int i = tid + 256 * j;
    obase[j] = -1;
    if (use_box && i < bxr.nx * bxr.ny) {
      const int ry = i / bxr.nx, rx = i - ry * bxr.nx;
      obase[j] = (ry + 1) * cw + rx + 1;
    }
  }
  const float* gxb = a.gx + 8 * c;
  // software pipeline: the global operands of plane k + 1 (dL/dt1 halo, t1, dL/dx, the source
  // gathers) are loaded while plane k is computed
  const int hi0 = tid, hi1 = tid + 256;
  auto halo = [&](int i, size_t kbv) {
    const int hy = i / 18, hx = i % 18, gy = ty0 - 1 + hy, gxx = tx0 - 1 + hx;
    return (i < 18 * 18 && gy >= 0 && gy < H && gxx >= 0 && gxx < W)
               ? coh_ld4(reinterpret_cast<const float*>(a.gt1 + kbv * HW + gy * W + gxx))
               : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  float4 nh0, nh1, ngx0, ngx1, ns[4][2];
  float nw = 0.f;
  TapF ntf;
  auto fetch = [&](int k) {
    const size_t kbv = ((size_t)k * pa.B + b) * nsrc + v;
    nh0 = halo(hi0, kbv);
    nh1 = halo(hi1, kbv);
    if (in) {
      nw = coh_ld(a.w + kbv * HW + p);
      const float* gxp = gxb + (((size_t)k * pa.B + b) * HW + p) * kC;
      ngx0 = coh_ld4(gxp);
      ngx1 = coh_ld4(gxp + 4);
      ntf = tap_f(m, pa.dvals[b * pa.D + a.d0 + k], x, y, H, W);
      const Box none{0, 0, 0, 0};
      const TapP t = tap_p(ntf, true, H, W, false, none, fbytes / 32u);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (AARMVS_CBF_ABL & 4) {
          ns[q][0] = ns[q][1] = make_float4(ntf.wt[0], ntf.wt[1], (float)t.pix[q], 0.f);
          continue;
        }
        ns[q][0] = ld_c8(rsrc, t.pix[q], 2 * c, HW);
        ns[q][1] = ld_c8(rsrc, t.pix[q], 2 * c + 1, HW);
      }
    }
  };
  fetch(0);
#pragma unroll 1
  for (int k = 0; k < a.n; ++k) {
    __syncthreads();   // cells zeroed / previous plane's LDS reads done
    gts[hi0] = nh0;
    if (hi1 < 18 * 18) gts[hi1] = nh1;
    if (mycell >= 0) cnt[mycell] = 0;
    mycell = -1;
    __syncthreads();
    const float wk = nw;
    const float4 gx0 = ngx0, gx1 = ngx1;
    const TapF tf = ntf;
    float4 sv4[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sv4[q][0] = ns[q][0];
      sv4[q][1] = ns[q][1];
    }
    if (k + 1 < a.n) fetch(k + 1);
    float sqv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float gw[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (in) {
      const Box none{0, 0, 0, 0};
      const TapP t = tap_p(tf, true, H, W, false, none, fbytes / 32u);
      const float4 g0 = bil4(sv4[0][0], sv4[1][0], sv4[2][0], sv4[3][0], t);
      const float4 g1 = bil4(sv4[0][1], sv4[1][1], sv4[2][1], sv4[3][1], t);
      const float4 s0 = sqdiff4(g0, rf0), s1 = sqdiff4(g1, rf1);
      const float wv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const float rv[8] = {rf0.x, rf0.y, rf0.z, rf0.w, rf1.x, rf1.y, rf1.z, rf1.w};
      sqv[0] = s0.x; sqv[1] = s0.y; sqv[2] = s0.z; sqv[3] = s0.w;
      sqv[4] = s1.x; sqv[5] = s1.y; sqv[6] = s1.z; sqv[7] = s1.w;
      const float gxv[8] = {gx0.x, gx0.y, gx0.z, gx0.w, gx1.x, gx1.y, gx1.z, gx1.w};
      const float dsc = -(wk + 1.0f) / (float)nsrc;
      float gsq[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) gsq[j] = dsc * gxv[j];
#pragma unroll 3
      for (int tap = 0; tap < ((AARMVS_CBF_ABL & 16) ? 1 : 9); ++tap) {
        const float4 gt = gts[(ly + 2 - tap / 3) * 18 + lx + 2 - tap % 3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float4 w = w0q[tap][j];
          gsq[j] = fmaf(w.x, gt.x, gsq[j]);
          gsq[j] = fmaf(w.y, gt.y, gsq[j]);
          gsq[j] = fmaf(w.z, gt.z, gsq[j]);
          gsq[j] = fmaf(w.w, gt.w, gsq[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        gw[j] = 2.0f * (wv[j] - rv[j]) * gsq[j];
        gref[j] -= gw[j];
      }
    }
    // grid_sample backward: file the pixel under its top-left tap's cell for the gather below;
    // taps that are never gathered (in-image corners outside the box, every corner of a pixel
    // outside the cells) are scattered with fixed-point global atomics here.  Whether a filed
    // pixel is gathered depends only on its cell's final count (read after the barrier), so the
    // result does not depend on the order the LDS atomics were served in.
    int kx = 0, ky = 0;
    if (in && !(AARMVS_CBF_ABL & 2) && tf.xf == tf.xf && tf.yf == tf.yf) {
      kx = (int)fminf(fmaxf(tf.xf, -8.f), (float)W + 8.f);
      ky = (int)fminf(fmaxf(tf.yf, -8.f), (float)H + 8.f);
      const int cx = kx - bxr.x0 + 1, cy = ky - bxr.y0 + 1;
      if (use_box && cx >= 0 && cx < cw && cy >= 0 && cy <= bxr.ny) {
        const int cell = cy * cw + cx;
        const int slot = atomicAdd(&cnt[cell], 1);
        mycell = cell;
        if (slot < kFbSlots) lst[cell][slot] = (unsigned short)tid;
        gwim[tid][0] = make_float4(gw[0], gw[1], gw[2], gw[3]);
        gwim[tid][1] = make_float4(gw[4], gw[5], gw[6], gw[7]);
        wtim[tid] = make_float4(tf.wt[0], tf.wt[1], tf.wt[2], tf.wt[3]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int xi = kx + (q & 1), yi = ky + (q >> 1);
        if (xi < 0 || xi >= W || yi < 0 || yi >= H) continue;   // zero padding
        const bool inbox = xi >= bxr.x0 && xi < bxr.x0 + bxr.nx && yi >= bxr.y0 && yi < bxr.y0 + bxr.ny;
        if (mycell >= 0 && inbox) continue;
        unsigned long long* gp = a.gsrc64 + ((((size_t)v * pa.B + b) * 4 + c) * HW + (size_t)yi * W + xi) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) atomicAdd(gp + j, to_fixed(tf.wt[q] * gw[j], fxk));
      }
    }
    sq4[tid][0] = make_float4(sqv[0], sqv[1], sqv[2], sqv[3]);
    sq4[tid][1] = make_float4(sqv[4], sqv[5], sqv[6], sqv[7]);
    __syncthreads();
    if (tid < kWgPairs * kWgSubs && !(AARMVS_CBF_ABL & 1)) {
      const int dy = ptap / 3, dx = ptap % 3;
#pragma unroll 4
      for (int qq = sub; qq < 256; qq += kWgSubs) {
        const float4 sv = sq4[qq][pcg];
        const float4 gt = gts[((qq >> 4) + 2 - dy) * 18 + (qq & 15) + 2 - dx];
        const float g4[4] = {gt.x, gt.y, gt.z, gt.w}, s4[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
        for (int co = 0; co < 4; ++co)
#pragma unroll
          for (int j = 0; j < 4; ++j) wacc[co * 4 + j] = fmaf(g4[co], s4[j], wacc[co * 4 + j]);
      }
    }
    // a cell holding more than kFbSlots pixels is not gathered: its pixels scatter their in-box
    // corners with the fixed-point atomics
    if (mycell >= 0 && cnt[mycell] > kFbSlots) {
      const float4 wq = wtim[tid], g0 = gwim[tid][0], g1 = gwim[tid][1];
      const float wt4[4] = {wq.x, wq.y, wq.z, wq.w};
      const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int xi = kx + (q & 1), yi = ky + (q >> 1);
        if (xi < 0 || xi >= W || yi < 0 || yi >= H) continue;
        const bool inbox = xi >= bxr.x0 && xi < bxr.x0 + bxr.nx && yi >= bxr.y0 && yi < bxr.y0 + bxr.ny;
        if (!inbox) continue;
        unsigned long long* gp = a.gsrc64 + ((((size_t)v * pa.B + b) * 4 + c) * HW + (size_t)yi * W + xi) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) atomicAdd(gp + j, to_fixed(wt4[q] * gv[j], fxk));
      }
    }
    // the gather: owned source pixel s takes corner q of the pixels filed under cell s - q, in
    // ascending tile-index order
    if (use_box && !(AARMVS_CBF_ABL & 2)) {
#pragma unroll
      for (int j = 0; j < kFbOwn; ++j) {
        if (obase[j] < 0) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cell = obase[j] - (q >> 1) * cw - (q & 1);
          const int n = cnt[cell];
          if (n > kFbSlots) continue;
          // ascending tile index by min / max: written for exactly two slots
          static_assert(kFbSlots == 2, "the fixed-order gather below sorts two slots");
          const int l0 = lst[cell][0], l1 = lst[cell][1];
          for (int sl = 0; sl < n; ++sl) {
            const int pp = n == 1 ? l0 : (sl == 0 ? min(l0, l1) : max(l0, l1));
            const float4 wq = wtim[pp];
            const float w = q == 0 ? wq.x : q == 1 ? wq.y : q == 2 ? wq.z : wq.w;
            const float4 g0 = gwim[pp][0], g1 = gwim[pp][1];
            own[j][0] += w * g0.x;
            own[j][1] += w * g0.y;
            own[j][2] += w * g0.z;
            own[j][3] += w * g0.w;
            own[j][4] += w * g1.x;
            own[j][5] += w * g1.y;
            own[j][6] += w * g1.z;
            own[j][7] += w * g1.w;
          }
        }
      }
    }
  }
  if (in) {
    float* gr = a.grefv + ((size_t)v * pa.B + b) * kC * HW + p;
#pragma unroll
    for (int j = 0; j < 8; ++j) coh_st(gr + (size_t)(8 * c + j) * HW, coh_ld(gr + (size_t)(8 * c + j) * HW) + gref[j]);
  }
  __syncthreads();   // every gather of the last plane done: the scratch becomes the subset sums
  if (tid < kWgPairs * kWgSubs) {
#pragma unroll
    for (int i = 0; i < 16; ++i) wsum[pair][sub][i] = wacc[i];
  }
  __syncthreads();
  if (use_box && !(AARMVS_CBF_ABL & 8)) {   // flush the owned box pixels (8 channels each)
    // through LDS (sq4's 8 KB, free after the last plane) so that consecutive lanes add to
    // consecutive channels: a wave-wide atomic covers 8 pixels x 64 B instead of 64 pixels'
    // separate lines
    unsigned long long* gb = a.gsrc64 + (((size_t)v * pa.B + b) * 4 + c) * HW * 8;
    float* fl = reinterpret_cast<float*>(sq4);
    const int nbox = bxr.nx * bxr.ny;
#pragma unroll
    for (int j = 0; j < kFbOwn; ++j) {
      if (256 * j >= nbox) break;   // block-uniform
      if (j > 0) __syncthreads();   // the previous round's reads done
      *reinterpret_cast<float4*>(fl + 8 * tid) = make_float4(own[j][0], own[j][1], own[j][2], own[j][3]);
      *reinterpret_cast<float4*>(fl + 8 * tid + 4) = make_float4(own[j][4], own[j][5], own[j][6], own[j][7]);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = tid + 256 * k, i = (e >> 3) + 256 * j, ch = e & 7;
        const float val = fl[e];
        if (i < nbox && val != 0.f) {
          const int ry = i / bxr.nx, rx = i - ry * bxr.nx;
          atomicAdd(gb + ((size_t)(bxr.y0 + ry) * W + bxr.x0 + rx) * 8 + ch, to_fixed(val, fxk));
        }
      }
    }
  }
  const int ntiles = tiles_x * ((H + kFbT - 1) / kFbT);
  const size_t blk = (((size_t)c * nsrc + v) * pa.B + b) * ntiles + tile;
  float* wp = a.wpart + blk * 288;
  for (int i = tid; i < 288; i += 256) {   // i = (co * 8 + j) * 9 + tap
    const int tap = i % 9, j = (i / 9) % 8, co = i / 72;
    const int pr = (j >> 2) * 9 + tap, col = co * 4 + (j & 3);
    float sum = wsum[pr][0][col];
#pragma unroll
    for (int k = 1; k < kWgSubs; ++k) sum += wsum[pr][k][col];
    wp[i] = sum;
  }
}

// per chunk c: sum the (view, b, tile) partials in a fixed order -> gW0[co][8c + j][tap], in
// two passes: 64 contiguous segments of the partials (blockIdx.y), then the segments in order.
constexpr int kW0Seg = 64;
__global__ void __launch_bounds__(256) cbw_w0_seg_kernel(const float* __restrict__ wpart, int nblk,
                                                         double* __restrict__ wseg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 1152) return;
  const int tap = i % 9, cc = (i / 9) % 32, co = i / 288;
  const int c = cc >> 3, j = cc & 7;
  const float* src = wpart + (size_t)c * nblk * 288 + (co * 8 + j) * 9 + tap;
  const int k0 = (int)((long)blockIdx.y * nblk / kW0Seg), k1 = (int)((long)(blockIdx.y + 1) * nblk / kW0Seg);
  double s = 0.0;
  for (int k = k0; k < k1; ++k) s += src[(size_t)k * 288];
  wseg[(size_t)blockIdx.y * 1152 + i] = s;
}

__global__ void __launch_bounds__(256) cbw_w0_reduce_kernel(const double* __restrict__ wseg,
                                                            double* __restrict__ gw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 1152) return;
  double s = 0.0;
  for (int k = 0; k < kW0Seg; ++k) s += wseg[(size_t)k * 1152 + i];
  gw[i] += s;
}

// dL/dref = sum over views (in view order) of the per-view accumulators
__global__ void __launch_bounds__(256) cbw_ref_sum_kernel(const float* __restrict__ grefv, int nsrc,
                                                          size_t n, float* __restrict__ gref) {
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float s = grefv[i];
    for (int v = 1; v < nsrc; ++v) s += grefv[(size_t)v * n + i];
    gref[i] = s;
  }
}

// c8 [B][4][HW][8] -> NCHW [B][32][HW]
__global__ void __launch_bounds__(256) c8_to_nchw_kernel(const float* __restrict__ src,
                                                         float* __restrict__ dst, int HW) {
  const int b = blockIdx.y;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < 32 * HW; i += gridDim.x * 256) {
    const int p = i % HW, ch = i / HW;
    dst[(size_t)b * 32 * HW + i] = src[(((size_t)b * 4 + (ch >> 3)) * HW + p) * 8 + (ch & 7)];
  }
}

// ---- host side ----
struct CostBwdLayout {
  float* go;
  float* wo;
  float4* gt1;
  double* gsum;
  double* part;
  float* wpart;
  double* wseg;
  float* gsrc8;
  float* grefv;
  unsigned long long* gsrc64;   // the current group's dL/dsrc in fixed point (cbw_feat_kernel)
  unsigned* gmax;               // [0] max |dL/dx|, [1] max |dL/dt1| of the group (float bits); then
  int* fxk;                     // the fixed-point exponent
  size_t bytes;
  int pblk, ntiles16;
};

static CostBwdLayout cost_bwd_layout(void* base, int B, int H, int W, int nsrc) {
  CostBwdLayout L{};
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off = (off + bytes + 255) / 256 * 256;
    return r;
  };
  const size_t HW = (size_t)H * W;
  const int G = kPlaneGroup;
  // blocks per (plane, b, view) of the chain kernels: a group launch has G x B x nsrc x pblk
  L.pblk = std::max(1, std::min((int)((HW + 4095) / 4096), 64));
  L.ntiles16 = ((W + kFbT - 1) / kFbT) * ((H + kFbT - 1) / kFbT);
  L.go = reinterpret_cast<float*>(take((size_t)G * B * nsrc * HW * 4));
  L.wo = reinterpret_cast<float*>(take((size_t)G * B * nsrc * HW * 4));
  L.gt1 = reinterpret_cast<float4*>(take((size_t)G * B * nsrc * HW * 16));
  L.gsum = reinterpret_cast<double*>(take((size_t)G * B * nsrc * 6 * 8));
  L.part = reinterpret_cast<double*>(take((size_t)G * B * nsrc * L.pblk * 32 * 8));
  L.wpart = reinterpret_cast<float*>(take((size_t)4 * nsrc * B * L.ntiles16 * 288 * 4));
  L.wseg = reinterpret_cast<double*>(take((size_t)kW0Seg * 1152 * 8));
  L.gsrc8 = reinterpret_cast<float*>(take((size_t)nsrc * B * 32 * HW * 4));
  L.grefv = reinterpret_cast<float*>(take((size_t)nsrc * B * 32 * HW * 4));
  L.gsrc64 = reinterpret_cast<unsigned long long*>(take((size_t)nsrc * B * 32 * HW * 8));
  L.gmax = reinterpret_cast<unsigned*>(take(256));
  L.fxk = reinterpret_cast<int*>(L.gmax ? L.gmax + 4 : nullptr);
  L.bytes = off;
  return L;
}

size_t cost_bwd_scratch_bytes(int B, int H, int W, int nsrc) {
  return cost_bwd_layout(nullptr, B, H, W, nsrc).bytes;
}

static CostArgs cost_args_of(const aarmvs_backward_args* a) {
  CostArgs ca{};
  ca.ref = a->ref_fea;
  for (int v = 0; v < a->nsrc; ++v) ca.src[v] = a->src_fea[v];
  ca.rel = a->rel_proj;
  ca.depth_values = a->depth_values;
  ca.params = static_cast<const float*>(a->packed_params);
  return ca;
}

hipError_t cost_bwd_begin(CostBwdCtx& c, hipStream_t s) {
  const aarmvs_backward_args* a = c.a;
  CostBwdLayout L = cost_bwd_layout(c.scratch, a->B, a->H, a->W, a->nsrc);
  hipError_t e;
  const size_t HW = (size_t)a->H * a->W;
  if ((e = hipMemsetAsync(L.gsrc8, 0, (size_t)a->nsrc * a->B * 32 * HW * 4, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(L.gsrc64, 0, (size_t)a->nsrc * a->B * 32 * HW * 8, s)) != hipSuccess) return e;
  return hipMemsetAsync(L.grefv, 0, (size_t)a->nsrc * a->B * 32 * HW * 4, s);
}

hipError_t cost_bwd_group(void* ctx, int g0, int n, const float* gx, hipStream_t s) {
  CostBwdCtx& c = *static_cast<CostBwdCtx*>(ctx);
  const aarmvs_backward_args* a = c.a;
  const ParamLayout& PL = param_layout();
  CostBwdLayout L = cost_bwd_layout(c.scratch, a->B, a->H, a->W, a->nsrc);
  const SweepGeom g{a->B, a->H, a->W, a->nsrc, a->D, cu_count()};
  const CostArgs ca = cost_args_of(a);
  hipError_t e;
  // the forward's omega conv output and GroupNorm statistics of the group's planes, read where
  // the recorded forward wrote them (the record's per-plane layout is the workspace slots')
  Workspace ws = c.ws;
  ws.t1 = a->record->t1 + (size_t)g0 * c.ws.t1_plane * 4;
  ws.omega_stats = a->record->ostats + (size_t)g0 * (c.ws.omega_stats_bytes / 8);
  CbwArgs ba{};
  ba.p = pipe_args_c8(ca, g, ws);
  group_strides(ba.p, ws, n);
  ba.p.t1_prev = reinterpret_cast<const float4*>(ws.t1);
  ba.p.st_prev = ws.omega_stats;
  ba.gx = gx;
  ba.go = L.go;
  ba.wo = L.wo;
  ba.gt1 = L.gt1;
  ba.gsum = L.gsum;
  ba.part = L.part;
  ba.gmax = L.gmax;
  ba.d0 = g0;
  ba.pblk = L.pblk;
  if ((e = hipMemsetAsync(L.gmax, 0, 8, s)) != hipSuccess) return e;
  const dim3 grid(L.pblk, a->nsrc, a->B * n);
  const int nkbv = n * a->B * a->nsrc, nrow = nkbv * L.pblk;
  auto cols = [&](int c0, std::initializer_list<std::pair<int, int>> ranges) {
    CbwCols cc{};
    cc.c0 = c0;
    int j = 0;
    for (const auto& r : ranges)
      for (int i = 0; i < r.second; ++i) cc.off[j++] = (int)PL.raw_off[r.first] + i;
    cc.ncol = j;
    return cc;
  };
  // stage 1: dL/do, GN3 sums; Wo, bo, gamma3, beta3
  {
    ProfScope ps(s, K_CBW_CHAIN);
    hipLaunchKernelGGL(cbw_chain_kernel<1>, grid, dim3(256), 0, s, ba, ba.p.params, ba.p.rel);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  { ProfScope ps_(s, K_CBW_SMALL);
  hipLaunchKernelGGL(cbw_gsum_kernel, dim3(nkbv), dim3(64), 0, s, L.part, L.pblk, L.gsum, 2);
  }
  {
    const CbwCols cc = cols(2, {{P_OWO, 4}, {P_OBO, 1}, {P_OG2W, 4}, {P_OG2B, 4}});
    { ProfScope ps_(s, K_CBW_SMALL);
    hipLaunchKernelGGL(cbw_param_kernel, dim3(cc.ncol), dim3(256), 0, s, L.part, nrow, cc, c.gacc);
    }
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // stage 2: GN2 sums; W2, b2, gamma2, beta2
  {
    ProfScope ps(s, K_CBW_CHAIN);
    hipLaunchKernelGGL(cbw_chain_kernel<2>, grid, dim3(256), 0, s, ba, ba.p.params, ba.p.rel);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  { ProfScope ps_(s, K_CBW_SMALL);
  hipLaunchKernelGGL(cbw_gsum_kernel, dim3(nkbv), dim3(64), 0, s, L.part, L.pblk, L.gsum, 1);
  }
  {
    const CbwCols cc = cols(2, {{P_OW2, 16}, {P_OB2, 4}, {P_OG1W, 4}, {P_OG1B, 4}});
    { ProfScope ps_(s, K_CBW_SMALL);
    hipLaunchKernelGGL(cbw_param_kernel, dim3(cc.ncol), dim3(256), 0, s, L.part, nrow, cc, c.gacc);
    }
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // stage 3: GN1 sums; W1, b1, gamma1, beta1
  {
    ProfScope ps(s, K_CBW_CHAIN);
    hipLaunchKernelGGL(cbw_chain_kernel<3>, grid, dim3(256), 0, s, ba, ba.p.params, ba.p.rel);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  { ProfScope ps_(s, K_CBW_SMALL);
  hipLaunchKernelGGL(cbw_gsum_kernel, dim3(nkbv), dim3(64), 0, s, L.part, L.pblk, L.gsum, 0);
  }
  {
    const CbwCols cc = cols(2, {{P_OW1, 16}, {P_OB1, 4}, {P_OG0W, 4}, {P_OG0B, 4}});
    { ProfScope ps_(s, K_CBW_SMALL);
    hipLaunchKernelGGL(cbw_param_kernel, dim3(cc.ncol), dim3(256), 0, s, L.part, nrow, cc, c.gacc);
    }
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // stage 4: dL/dt1; b0
  {
    ProfScope ps(s, K_CBW_CHAIN);
    hipLaunchKernelGGL(cbw_chain_kernel<4>, grid, dim3(256), 0, s, ba, ba.p.params, ba.p.rel);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  {
    const CbwCols cc = cols(0, {{P_OB0, 4}});
    { ProfScope ps_(s, K_CBW_SMALL);
    hipLaunchKernelGGL(cbw_param_kernel, dim3(cc.ncol), dim3(256), 0, s, L.part, nrow, cc, c.gacc);
    }
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // dL/dsq -> features, conv3x3 weights
  CbfArgs fa{};
  fa.p = ba.p;
  fa.gx = gx;
  fa.gt1 = L.gt1;
  fa.w = L.wo;
  fa.gsrc64 = L.gsrc64;
  fa.fxk = L.fxk;
  fa.grefv = L.grefv;
  {
    ProfScope ps_(s, K_CBW_SMALL);
    hipLaunchKernelGGL(cbw_scale_kernel, dim3(1), dim3(64), 0, s, L.gmax, c.ws.xbound,
                       ba.p.params + ba.p.off_ow0, a->H * a->W, n, a->nsrc, L.fxk);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  fa.wpart = L.wpart;
  fa.d0 = g0;
  fa.n = n;
  {
    ProfScope ps(s, K_CBW_FEAT);
    hipLaunchKernelGGL(cbw_feat_kernel, dim3(L.ntiles16 * 4 * a->nsrc, 1, a->B), dim3(256), 0, s, fa,
                       ba.p.params, ba.p.rel);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  { ProfScope ps_(s, K_CBW_SMALL);
  hipLaunchKernelGGL(cbw_w0_seg_kernel, dim3(5, kW0Seg), dim3(256), 0, s, L.wpart,
                     a->nsrc * a->B * L.ntiles16, L.wseg);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  { ProfScope ps_(s, K_CBW_SMALL);
  hipLaunchKernelGGL(cbw_w0_reduce_kernel, dim3(5), dim3(256), 0, s, L.wseg, c.gacc + PL.raw_off[P_OW0]);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  {
    const size_t nel = (size_t)a->nsrc * a->B * 32 * a->H * a->W;
    ProfScope ps_(s, K_CBW_SMALL);
    hipLaunchKernelGGL(cbw_fold_kernel, dim3((unsigned)std::min<size_t>(4096, (nel + 255) / 256)), dim3(256), 0, s,
                       L.gsrc64, L.gsrc8, nel, L.fxk);
  }
  }
  return hipGetLastError();
}

hipError_t cost_bwd_end(CostBwdCtx& c, hipStream_t s) {
  const aarmvs_backward_args* a = c.a;
  CostBwdLayout L = cost_bwd_layout(c.scratch, a->B, a->H, a->W, a->nsrc);
  const int HW = a->H * a->W;
  {
    const size_t n = (size_t)a->B * 32 * HW;
    hipLaunchKernelGGL(cbw_ref_sum_kernel, dim3((unsigned)std::min<size_t>(4096, (n + 255) / 256)), dim3(256),
                       0, s, L.grefv, a->nsrc, n, a->grad_ref);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  for (int v = 0; v < a->nsrc; ++v) {
    if (!a->grad_src[v]) continue;
    hipLaunchKernelGGL(c8_to_nchw_kernel, dim3(std::min(4096, (32 * HW + 255) / 256), a->B), dim3(256), 0, s,
                       L.gsrc8 + (size_t)v * a->B * 32 * HW, a->grad_src[v], HW);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace aarmvs
