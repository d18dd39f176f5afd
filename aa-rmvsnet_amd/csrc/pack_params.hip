// The packed parameter buffer (ParamLayout, aarmvs_internal.h): its layout, the kernels that
// pack the raw blob into it (aarmvs_pack_params) and the two size queries.
#include <hip/hip_runtime.h>

#include <cmath>

#include "aarmvs_internal.h"

namespace aarmvs {

const ParamLayout& param_layout() {
  static ParamLayout L = [] {
    ParamLayout l{};
    size_t raw = 0, pk = 0;
    for (int i = 0; i < P_COUNT; ++i) {
      l.raw_off[i] = raw;
      l.pk_off[i] = pk;
      raw += kParamSize[i];
      pk += ((size_t)kParamSize[i] + 63) / 64 * 64;
    }
    for (int k = 0; k < 5; ++k) {
      l.h3_off[k] = pk;
      pk += ((size_t)cell_a_halves(k) + 63) / 64 * 64;   // 2 x halves = halves floats
    }
    for (int k = 0; k < 5; ++k) {
      l.h3p_off[k] = pk;
      pk += ((size_t)cell_a_halves(k) + 63) / 64 * 64;
    }
    l.h3_scale_off = pk;
    pk += 64;
    l.ow0t_off = pk;
    pk += 4 * 32 * 9;
    l.owb_scale_off = pk;
    pk += 64;
    l.owm_off = pk;
    pk += 4 * 3 * 64 * 8 / 2;   // halves -> floats
    for (int k = 0; k < 2; ++k) {
      l.dct_off[k] = pk;
      pk += 16 * 9 * 16;
    }
    for (int k = 0; k < 2; ++k) {
      l.dcm_off[k] = pk;
      pk += 6 * 2 * 64 * 8 / 2 + 64;   // halves -> floats, then the scale (64-float aligned)
    }
    for (int k = 0; k < 5; ++k) {
      l.dg_off[k] = pk;
      pk += ((size_t)dg_mtiles(k) * dg_mt_halves(k) / 2 + 63) / 64 * 64;
    }
    l.dg_scale_off = pk;
    pk += 64;
    l.raw_total = raw;
    l.pk_total = pk;
    return l;
  }();
  return L;
}

// ---------------------------------------------------------------------------
// Parameter packing: cell weights [4*hid][cin][3][3] -> MFMA A operands
// [K/2][MT][64] with k = tap*cin + ci and m-tile row r -> cout (r>>3)*hid + 8*mt + (r&7).
// Everything else is copied (64-float aligned sections).
// ---------------------------------------------------------------------------
__global__ void pack_params_kernel(const float* __restrict__ raw, float* __restrict__ pk,
                                   ParamLayout L) {
  const int id = blockIdx.y;
  const int n = kParamSize[id];
  const float* src = raw + L.raw_off[id];
  float* dst = pk + L.pk_off[id];
  const bool is_cell_w = id >= P_C0W && id <= P_C4W && ((id - P_C0W) % 2 == 0);
  const int k = (id - P_C0W) / 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (!is_cell_w) {
      dst[i] = src[i];
      continue;
    }
    const int hid = kCellHid[k], cin = kCellCX[k] + hid, mt_n = hid / 8;
    const int l = i % 64, mt = (i / 64) % mt_n, s = i / (64 * mt_n);
    const int kk = 2 * s + (l >> 5);
    const int tap = kk / cin, ci = kk % cin;
    const int r = l & 31;
    const int cout = (r >> 3) * hid + 8 * mt + (r & 7);
    dst[i] = src[(cout * cin + ci) * 9 + tap];
  }
}

// Split-fp16 cell weights: w * 2^e = hi + lo (both fp16, hi = fp16(w 2^e),
// lo = fp16(w 2^e - hi)), e chosen per cell so that max|w| 2^e <= 2^14 (lo stays in
// fp16's normal range for all but tiny weights).  One block per cell.
__global__ void __launch_bounds__(256) pack_cell_h3_kernel(const float* __restrict__ raw,
                                                           float* __restrict__ pk, ParamLayout L) {
  __shared__ float red[4];
  const int k = blockIdx.x;
  const int hid = kCellHid[k], cin = cell_cin(k), cout = 4 * hid, mt_n = hid / 8;
  const float* w = raw + L.raw_off[P_C0W + 2 * k];   // [cout][cin][3][3]
  const int n = cout * cin * 9;
  float mx = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) mx = fmaxf(mx, fabsf(w[i]));
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int e = 0;
  if (mx > 0.f) {
    e = (int)floorf(log2f(16384.0f / mx));
    e = e < -20 ? -20 : (e > 20 ? 20 : e);
  }
  const float sc = ldexpf(1.0f, e);
  if (threadIdx.x == 0) pk[L.h3_scale_off + k] = ldexpf(1.0f, -e);
  const int halves = cell_a_halves(k);
  _Float16* hi = reinterpret_cast<_Float16*>(pk + L.h3_off[k]);
  _Float16* lo = hi + halves;
  _Float16* hip = reinterpret_cast<_Float16*>(pk + L.h3p_off[k]);
  _Float16* lop = hip + halves;
  for (int i = threadIdx.x; i < halves; i += blockDim.x) {
    const int j = i & 7, l = (i >> 3) & 63, rest = i >> 9;   // [chunk][tap][mt][lane][j]
    const int mt = rest % mt_n, tap = (rest / mt_n) % 9, c = rest / (mt_n * 9);
    const int r = l & 31, h = l >> 5;
    const int co = (r >> 3) * hid + 8 * mt + (r & 7);
    // a chunk of 8 valid channels is paired (convlstm.hip h3_mfma_chunk): its slot s < 5 holds
    // tap 2s (K half 0) and tap 2s+1 (K half 1) of those channels; slots 5..8 stay zero
    const bool paired = cin - 16 * c == 8;
    const int tp = paired ? 2 * tap + h : tap;
    const int ci = paired ? 16 * c + j : 16 * c + 8 * h + j;
    // slots with (slot + chunk) odd negated: the cells' sign-balanced accumulation (convlstm.hip)
    const bool neg = ((tap + c) & 1) != 0;
    const float v = ci < cin && tp < 9 ? w[(co * cin + ci) * 9 + tp] * sc : 0.f;
    const _Float16 vh = (_Float16)v, vl = (_Float16)(v - (float)vh);
    hip[i] = vh;
    lop[i] = vl;
    hi[i] = neg ? -vh : vh;   // (fp16 negation is exact: the balanced copy is the same split)
    lo[i] = neg ? -vl : vl;
  }
}

// omega conv3x3 32->4 weights [co][ci][tap] -> [tap][ci][co]: the 16 weights of one
// (tap, 4-channel group) are contiguous (scalar loads in the VALU form of the conv)
// and -> split-fp16 B fragments of v_mfma_f32_16x16x32_f16 for omega_conv's MFMA conv
// (the eight off-centre taps): per 8-channel chunk c and N tile k, column n = 4 u + co
// (tap slot u = 4 k + n / 4: taps 0..3, 5..8), k8 group g = lane / 16 against the A
// groups [sq hi | sq lo | sq hi | sq lo]: W hi for g < 2, W lo for g >= 2.  Lane l of
// fragment (c, k) holds B[8 g .. 8 g + 7][n = l % 16].  A power-of-two scale keeps the
// weights in fp16's normal range (undone in the kernel's epilogue).
__global__ void pack_omega_conv_kernel(const float* __restrict__ raw, float* __restrict__ pk,
                                       ParamLayout L) {
  __shared__ float red[4];
  const float* w = raw + L.raw_off[P_OW0];
  float* d = pk + L.ow0t_off;
  float mx = 0.f;
  for (int i = threadIdx.x; i < 4 * 32 * 9; i += blockDim.x) {
    const int co = i % 4, ci = (i / 4) % 32, tap = i / 128;
    d[i] = w[(co * 32 + ci) * 9 + tap];
    mx = fmaxf(mx, fabsf(d[i]));
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int e = 0;
  if (mx > 0.f) {
    e = (int)floorf(log2f(16384.0f / mx));
    e = e < -20 ? -20 : (e > 20 ? 20 : e);
  }
  const float sc = ldexpf(1.0f, e);
  if (threadIdx.x == 0) pk[L.owb_scale_off] = ldexpf(1.0f, -e);
  // omega_mfma's v_mfma_f32_32x32x16_f16 B fragments: per chunk c and kind k against
  // A = [sq hi | sq lo]: 0: [W_hi; W_hi], 1: [W_lo; 0], 2: [W_lo2; W_lo] with W = W_hi + W_lo +
  // W_lo2 (three fp16 terms: the weights exact to ~2^-33, so the conv carries no systematic
  // per-weight error; the dropped terms are sq_lo W_lo2 and sq_lo's own rounding, ~2^-22 random
  // per product); lane l holds B[8 (l >> 5) + j][n = l & 31] with column n = 4 u + co.  The
  // kernel passes them as the A operand (the product transposed: rows n, columns pixels), so
  // that slot u of row group g = u >> 1 lands in accumulator registers 4 g .. 4 g + 3 of lanes
  // 0-31 (u even) or 32-63 (u odd); tap slots u -> taps 0, 6, 1, 7, 2, 8, 3, 5 pair the taps of
  // one dx in one register group (omega_item's row sums)
  _Float16* bm = reinterpret_cast<_Float16*>(pk + L.owm_off);
  for (int i = threadIdx.x; i < 4 * 3 * 64 * 8; i += blockDim.x) {
    const int j = i & 7, lane = (i >> 3) & 63, k = (i >> 9) % 3, c = (i >> 9) / 3;
    const int n = lane & 31, u = n >> 2, g = u >> 1, co = n & 3;
    const int tap = (u & 1) ? (g < 3 ? 6 + g : 5) : g;
    const float x = w[(co * 32 + 8 * c + j) * 9 + tap] * sc;
    const _Float16 xh = (_Float16)x;
    const float r1 = x - (float)xh;
    const _Float16 xl = (_Float16)r1;
    const _Float16 xl2 = (_Float16)(r1 - (float)xl);
    const bool top = (lane >> 5) == 0;   // K rows 0-7: against sq hi
    bm[i] = k == 0 ? xh : k == 1 ? (top ? xl : (_Float16)0.0f) : (top ? xl2 : xl);
  }
}

// deconv weights [ci][co][ky][kx] (ConvTranspose2d) -> [ci][tap][co]: the 16 output
// channels of one (ci, tap) are contiguous, so the deconv's packed FMAs pair adjacent
// scalar registers
__global__ void pack_deconv_kernel(const float* __restrict__ raw, float* __restrict__ pk,
                                   ParamLayout L) {
  const int k = blockIdx.x;
  const float* w = raw + L.raw_off[k ? P_D1W : P_D0W];
  float* d = pk + L.dct_off[k];
  for (int i = threadIdx.x; i < 16 * 9 * 16; i += blockDim.x) {
    const int co = i % 16, tap = (i / 16) % 9, ci = i / 144;
    d[i] = w[(ci * 16 + co) * 9 + tap];
  }
}

// deconv_0/1 as split-fp16 MFMA A fragments (deconv_mfma_kernel): six tap pairs, rows
// m = slot * 16 + co (slot 0 / 1: the two output pixels of a pair), k = ci; lane l holds row
// l & 31, input channels 8 (l >> 5) .. +7.  Pairs (tap of slot 0 | slot 1, input pixel):
// (4 | 5, v00), (- | 3, v01), (7 | 8, v00), (- | 6, v01), (1 | 2, v10), (- | 0, v11) -- the
// ConvTranspose2d(k3, s2, p1, op1) taps feeding output (2y + a, 2x + b) from input (y, x)
// and its right / lower neighbours.  Values are scaled by 2^e (max |w| 2^e < 2^15).
__global__ void pack_deconv_mfma_kernel(const float* __restrict__ raw, float* __restrict__ pk,
                                        ParamLayout L) {
  __shared__ float red[4];
  const int k = blockIdx.x;
  const float* w = raw + L.raw_off[k ? P_D1W : P_D0W];   // [ci][co][3][3]
  float mx = 0.f;
  for (int i = threadIdx.x; i < 16 * 16 * 9; i += blockDim.x) mx = fmaxf(mx, fabsf(w[i]));
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const int e = mx > 0.f ? 14 - ilogbf(mx) : 0;
  const float sc = ldexpf(1.0f, e);
  constexpr int kTap[6][2] = {{4, 5}, {-1, 3}, {7, 8}, {-1, 6}, {1, 2}, {-1, 0}};
  _Float16* f = reinterpret_cast<_Float16*>(pk + L.dcm_off[k]);
  for (int i = threadIdx.x; i < 6 * 64 * 8; i += blockDim.x) {
    const int j = i & 7, lane = (i >> 3) & 63, pair = i >> 9;
    const int m = lane & 31, slot = m >> 4, co = m & 15, ci = 8 * (lane >> 5) + j;
    const int tap = kTap[pair][slot];
    const float v = tap < 0 ? 0.f : w[(ci * 16 + co) * 9 + tap] * sc;
    const _Float16 hi = (_Float16)v;
    f[((pair * 2 + 0) * 64 + lane) * 8 + j] = hi;
    f[((pair * 2 + 1) * 64 + lane) * 8 + j] = (_Float16)(v - (float)hi);
  }
  if (threadIdx.x == 0) pk[L.dcm_off[k] + 6 * 2 * 64 * 8 / 2] = ldexpf(1.0f, -e);
}

// BPTT input-gradient conv of each cell: dL/d[input] = conv3x3(dL/dz) with the forward
// weight W[cz][ci][tap] (cz: gate channel, ci: input channel) transposed and flipped,
// A[ci][cz, tap] = W[cz][ci][8 - tap].  Fragments [m-tile][chunk][tap][hi, lo][lane][8]: lane l
// holds row ci = 32 mt + (l & 31), gate channels 16 chunk + 8 (l >> 5) .. +7; rows past cin are
// zero.  Power-of-two scale per cell as for the forward fragments.  One block per cell.
__global__ void __launch_bounds__(256) pack_dgrad_kernel(const float* __restrict__ raw,
                                                         float* __restrict__ pk, ParamLayout L) {
  __shared__ float red[4];
  const int k = blockIdx.x;
  const int hid = kCellHid[k], cin = cell_cin(k), cz = 4 * hid;
  const float* w = raw + L.raw_off[P_C0W + 2 * k];   // [cz][cin][3][3]
  const int n = cz * cin * 9;
  float mx = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) mx = fmaxf(mx, fabsf(w[i]));
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  int e = 0;
  if (mx > 0.f) {
    e = (int)floorf(log2f(16384.0f / mx));
    e = e < -20 ? -20 : (e > 20 ? 20 : e);
  }
  const float sc = ldexpf(1.0f, e);
  if (threadIdx.x == 0) pk[L.dg_scale_off + k] = ldexpf(1.0f, -e);
  const int nch = dg_chunks(k), mtn = dg_mtiles(k);
  _Float16* f = reinterpret_cast<_Float16*>(pk + L.dg_off[k]);
  const int total = mtn * dg_mt_halves(k);
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int j = i & 7, l = (i >> 3) & 63, hl = (i >> 9) & 1, rest = i >> 10;
    const int tap = rest % 9, c = (rest / 9) % nch, mt = rest / (9 * nch);
    const int ci = 32 * mt + (l & 31), z = 16 * c + 8 * (l >> 5) + j;
    // taps with (tap + chunk) odd negated: dgrad's sign-balanced accumulation (bptt.hip)
    const float sg = ((tap + c) & 1) ? -1.0f : 1.0f;
    const float v = ci < cin ? w[(z * cin + ci) * 9 + (8 - tap)] * sc * sg : 0.f;
    const _Float16 vh = (_Float16)v;
    f[i] = hl == 0 ? vh : (_Float16)(v - (float)vh);
  }
}

hipError_t launch_pack_params(const float* raw, float* packed, hipStream_t s) {
  const ParamLayout& L = param_layout();
  hipError_t e = hipMemsetAsync(packed, 0, L.pk_total * sizeof(float), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pack_params_kernel, dim3(32, P_COUNT), dim3(256), 0, s, raw, packed, L);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pack_cell_h3_kernel, dim3(5), dim3(256), 0, s, raw, packed, L);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pack_omega_conv_kernel, dim3(1), dim3(256), 0, s, raw, packed, L);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pack_deconv_kernel, dim3(2), dim3(256), 0, s, raw, packed, L);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pack_deconv_mfma_kernel, dim3(2), dim3(256), 0, s, raw, packed, L);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pack_dgrad_kernel, dim3(5), dim3(256), 0, s, raw, packed, L);
  return hipGetLastError();
}

}  // namespace aarmvs

using namespace aarmvs;

extern "C" {

size_t aarmvs_param_count(void) { return param_layout().raw_total; }
size_t aarmvs_packed_param_bytes(void) { return param_layout().pk_total * sizeof(float); }

int aarmvs_pack_params(const float* raw_params, void* packed, hipStream_t stream) {
  if (!raw_params || !packed) return fail(AARMVS_ERR_INVALID, "pack_params: null pointer");
  return launched(launch_pack_params(raw_params, static_cast<float*>(packed), stream), "pack_params");
}

}  // extern "C"
