// C-ABI entry points of libaarmvs (include/aarmvs.h): argument validation, the
// parameter packing kernel, the workspace carve and the per-plane sweep schedule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "aarmvs_internal.h"

namespace aarmvs {

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

static int hip_fail(hipError_t e, const char* where) {
  return fail(AARMVS_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

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
// Opt-in kernel timer (aarmvs_profile_*).  Events come from a pool that grows to
// the largest profiling window and is reused after aarmvs_profile_reset.
// ---------------------------------------------------------------------------
bool g_prof_on = false;
static std::mutex g_prof_mu;
static std::vector<hipEvent_t> g_prof_pool;
static size_t g_prof_used = 0;
struct ProfRec {
  int id;
  hipEvent_t a, b;
};
static std::vector<ProfRec> g_prof_recs;
static hipEvent_t g_prof_open[K_COUNT];
static double g_prof_ms[K_COUNT];
static long long g_prof_n[K_COUNT];

static const char* kKernelNames[K_COUNT] = {
    "cost_x", "omega_conv", "fusion", "omega_stats1", "omega_stats2",
    "lstm_cell0", "lstm_cell1", "lstm_cell2", "lstm_cell3", "lstm_cell4",
    "deconv0", "deconv1", "head_wta", "finalize", "softmax_depth", "homo_warp", "to_c8",
    "omega_stat_reduce", "gn_reduce", "evidential",
    "gate_bwd0", "gate_bwd1", "gate_bwd2", "gate_bwd3", "gate_bwd4",
    "dgrad0", "dgrad1", "dgrad2", "dgrad3", "dgrad4",
    "wgrad0", "wgrad1", "wgrad2", "wgrad3", "wgrad4",
    "gnb_partial", "deconv_bwd", "bwd_small", "cbw_chain", "cbw_feat", "cbw_small",
    "deconv_wgrad", "head_wgrad", "deform_sample",
    "pyr_down", "fusion_points",
    "cls_loss_fwd", "cls_loss_reduce", "cls_loss_bwd", "depth_metrics",
    "lstm_cell0_fp16", "lstm_cell1_fp16", "lstm_cell2_fp16", "lstm_cell3_fp16", "lstm_cell4_fp16",
    "deconv0_fp16", "deconv1_fp16", "refine"};

static hipEvent_t prof_event() {
  if (g_prof_used == g_prof_pool.size()) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    g_prof_pool.push_back(e);
  }
  return g_prof_pool[g_prof_used++];
}

void prof_mark(hipStream_t s, int id, bool begin) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  hipEvent_t e = prof_event();
  if (!e) return;
  (void)hipEventRecord(e, s);
  if (begin) {
    g_prof_open[id] = e;
  } else if (g_prof_open[id]) {
    g_prof_recs.push_back({id, g_prof_open[id], e});
    g_prof_open[id] = nullptr;
  }
}

static void prof_fold() {
  for (const ProfRec& r : g_prof_recs) {
    float ms = 0.f;
    if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      g_prof_ms[r.id] += ms;
      g_prof_n[r.id] += 1;
    }
  }
  g_prof_recs.clear();
  g_prof_used = 0;
}

int cu_count() {
  static int cu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      return 256;
    return n;
  }();
  return cu;
}

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

Workspace carve_workspace(void* base, int B, int H, int W, int nsrc) {
  Workspace ws{};
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + off : nullptr;
    off = align_up(off + bytes, 256);
    return r;
  };
  const size_t HW = (size_t)H * W, HW2 = HW / 4, HW4 = HW / 16;
  ws.omega_stats_bytes = (size_t)B * nsrc * 3 * kSlots * 2 * sizeof(double);
  ws.reg_stats_bytes = (size_t)B * 4 * kSlots * 2 * sizeof(double);
  const size_t stats_begin = off;
  ws.omega_stats = reinterpret_cast<double*>(take(kPlaneGroup * ws.omega_stats_bytes));
  ws.reg_stats = reinterpret_cast<double*>(take(ws.reg_stats_bytes));
  ws.xbound = reinterpret_cast<unsigned*>(take(sizeof(unsigned)));
  ws.stats_bytes = off - stats_begin;
  const size_t wta_begin = off;
  ws.max_prob = reinterpret_cast<float*>(take(B * HW * 4));
  ws.exp_sum = reinterpret_cast<float*>(take(B * HW * 4));
  ws.depth = reinterpret_cast<float*>(take(B * HW * 4));
  ws.wta_bytes = off - wta_begin;
  ws.x_plane = (size_t)B * kC * HW;
  ws.t1_plane = (size_t)B * nsrc * HW;
  ws.xg[0] = reinterpret_cast<float*>(take(kPlaneGroup * ws.x_plane * 4));
  ws.xg[1] = reinterpret_cast<float*>(take(kPlaneGroup * ws.x_plane * 4));
  ws.x = ws.xg[0];
  for (int v = 0; v <= nsrc; ++v) ws.feat8[v] = reinterpret_cast<float*>(take(B * kC * HW * 4));
  ws.t1 = reinterpret_cast<float*>(take(kPlaneGroup * ws.t1_plane * 16));
  // one partial per omega block (haloed 16 x TW tiles, 14 x (TW - 2) outputs, TW >= 16; the
  // VALU variant's 16 x 32 output tiles are fewer) or statistics block (<= one per 1024 px)
  ws.omega_part_n = (int)std::max(((size_t)(W + 13) / 14) * ((size_t)(H + 13) / 14), (HW + 1023) / 1024);
  ws.omega_part = reinterpret_cast<double*>(
      take((size_t)kPlaneGroup * B * nsrc * ws.omega_part_n * 2 * sizeof(double)));
  // deconv_1's blocks (8 x 32 tiles of its H/2 x W/2 input) outnumber deconv_0's
  ws.reg_part = reinterpret_cast<double*>(
      take((size_t)B * ((W / 2 + 31) / 32) * ((H / 2 + 7) / 8) * 4 * sizeof(double)));
  ws.reg_part0 = reinterpret_cast<double*>(
      take((size_t)B * ((W / 4 + 31) / 32) * ((H / 4 + 7) / 8) * 4 * sizeof(double)));
  ws.u0 = reinterpret_cast<float*>(take(B * 16 * HW2 * 4));
  ws.u1 = reinterpret_cast<float*>(take(B * 16 * HW * 4));
  const size_t state_begin = off;
  ws.state_begin = p ? p + off : nullptr;
  const size_t cell_px[5] = {HW, HW2, HW4, HW2, HW};
  for (int k = 0; k < 5; ++k) {
    const size_t n = (size_t)B * kCellHid[k] * cell_px[k] * 4;
    for (int r = 0; r < kHRingMax; ++r) ws.h[k][r] = r < kHRing[k] ? reinterpret_cast<float*>(take(n)) : nullptr;
    ws.c[k] = reinterpret_cast<float*>(take(n));
  }
  ws.state_bytes = off - state_begin;
  for (int k = 0; k < 2; ++k)
    for (int r = 0; r < kHRingMax; ++r)
      ws.h_pool[k][r] = r < kHRing[k] ? reinterpret_cast<float*>(take((size_t)B * kCellHid[k] * (cell_px[k] / 4) * 4))
                                      : nullptr;
  ws.bytes = off;
  return ws;
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

const char* aarmvs_last_error(void) { return g_err.c_str(); }

void aarmvs_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
}

void aarmvs_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  prof_fold();
  for (int i = 0; i < K_COUNT; ++i) {
    g_prof_ms[i] = 0.0;
    g_prof_n[i] = 0;
    g_prof_open[i] = nullptr;
  }
}

int aarmvs_profile_kernel_count(void) { return K_COUNT; }

const char* aarmvs_profile_kernel_name(int id) {
  return (id >= 0 && id < K_COUNT) ? kKernelNames[id] : nullptr;
}

int aarmvs_profile_read(int id, long long* launches, double* total_ms) {
  if (id < 0 || id >= K_COUNT || !launches || !total_ms)
    return fail(AARMVS_ERR_INVALID, "profile_read: bad arguments");
  std::lock_guard<std::mutex> lk(g_prof_mu);
  prof_fold();
  *launches = g_prof_n[id];
  *total_ms = g_prof_ms[id];
  return AARMVS_OK;
}
const char* aarmvs_version(void) { return "aarmvs-mi355x 0.1 (gfx950)"; }

size_t aarmvs_param_count(void) { return param_layout().raw_total; }
size_t aarmvs_packed_param_bytes(void) { return param_layout().pk_total * sizeof(float); }

int aarmvs_pack_params(const float* raw_params, void* packed, hipStream_t stream) {
  if (!raw_params || !packed) return fail(AARMVS_ERR_INVALID, "pack_params: null pointer");
  hipError_t e = launch_pack_params(raw_params, static_cast<float*>(packed), stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "pack_params");
}

int aarmvs_homo_warp(const float* src_fea, const float* rel_proj, const float* depth, int B,
                     int C, int H, int W, float* out, hipStream_t stream) {
  if (!src_fea || !rel_proj || !depth || !out) return fail(AARMVS_ERR_INVALID, "homo_warp: null pointer");
  if (B < 1 || C < 1 || H < 2 || W < 2)
    return fail(AARMVS_ERR_INVALID, "homo_warp: need B>=1, C>=1, H>=2, W>=2");
  hipError_t e = launch_homo_warp(src_fea, rel_proj, depth, B, C, H, W, out, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "homo_warp");
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
  hipError_t e = launch_homo_warp_bwd(grad_out, rel_proj, depth, B, C, H, W, grad_src, workspace, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "homo_warp_backward");
}

static int check_geom(int B, int H, int W, int nsrc) {
  if (B < 1) return fail(AARMVS_ERR_INVALID, "B must be >= 1");
  if (H < 4 || W < 4 || H % 4 || W % 4)
    return fail(AARMVS_ERR_INVALID,
                "H and W must be positive multiples of 4 (two 2x2 pools + two stride-2 deconvs)");
  if (nsrc < 1 || nsrc > AARMVS_MAX_SRC)
    return fail(AARMVS_ERR_INVALID, "nsrc must be in [1, AARMVS_MAX_SRC]");
  // the pipeline kernels address one view's 32-channel image with 32-bit byte offsets and
  // the per-view maps with 32-bit element indices
  const long long hw = (long long)H * W;
  if (hw * 128 >= (1ll << 32) || (long long)B * (nsrc + 1) * hw >= (1ll << 31))
    return fail(AARMVS_ERR_INVALID, "H x W (x B x views) too large for 32-bit image offsets");
  return AARMVS_OK;
}

size_t aarmvs_sweep_workspace_bytes(int B, int H, int W, int nsrc) {
  if (check_geom(B, H, W, nsrc) != AARMVS_OK) return 0;
  return carve_workspace(nullptr, B, H, W, nsrc).bytes;
}

size_t aarmvs_train_record_bytes(int B, int H, int W, int which) {
  if (check_geom(B, H, W, 1) != AARMVS_OK) return 0;
  const TrainLayout T = train_layout(B, H, W);
  switch (which) {
    case 0: return T.x_plane * sizeof(float);
    case 1: return T.state_slab * sizeof(float);
    case 2: return T.z_slab * sizeof(float);
    case 3: return T.u_slab * sizeof(float);
    case 4: return T.stats_slab * sizeof(double);
    case 5: return (size_t)B * H * W * 16;                        // t1 of one view
    case 6: return (size_t)B * 3 * kSlots * 2 * sizeof(double);   // omega statistics of one view
    default: return 0;
  }
}

int aarmvs_train_segment_bytes(int B, int H, int W, int nsrc, int planes, size_t* record_bytes,
                               size_t* checkpoint_bytes) {
  int rc = check_geom(B, H, W, nsrc);
  if (rc) return rc;
  if (planes < 1) return fail(AARMVS_ERR_INVALID, "train_segment_bytes: planes must be >= 1");
  const size_t n = (size_t)planes;
  size_t total = 0;
  for (int which = 0; which < 7; ++which) {
    const size_t slabs = which == 1 ? n + 1 : which >= 5 ? n * nsrc : n;
    total += slabs * aarmvs_train_record_bytes(B, H, W, which);
  }
  if (record_bytes) *record_bytes = total;
  if (checkpoint_bytes) *checkpoint_bytes = aarmvs_train_record_bytes(B, H, W, 1);
  return AARMVS_OK;
}

int aarmvs_aux_stream(hipStream_t* out) {
  if (!out) return fail(AARMVS_ERR_INVALID, "aux_stream: null out");
  int dev = 0;
  hipError_t e = current_device(dev);
  if (e == hipSuccess) e = library_stream(dev, kLibStreams, *out);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "aux_stream");
}

float* aarmvs_state_ptr(void* workspace, int B, int H, int W, int nsrc, int planes,
                        int cell, int which) {
  if (!workspace || cell < 0 || cell > 4 || planes < 0 || check_geom(B, H, W, nsrc) != AARMVS_OK)
    return nullptr;
  Workspace ws = carve_workspace(workspace, B, H, W, nsrc);
  return which == 0 ? ws.h[cell][h_slot(cell, planes)] : ws.c[cell];
}

}  // extern "C"

// The sweep's stream schedule is sweep_schedule.h: plan_sweep chooses the streams, walk_sweep
// gives the order of the launches, records and waits, aarmvs_sweep executes them.
static_assert(kLib4 - kLib1 + 1 == kLibStreams && kRegMaxStreams - 1 == kLibStreams,
              "unit streams 1..3 are library streams 1..3; a fifth unit stream is library stream "
              "4, the stream aarmvs_aux_stream returns");
// the overrides of a call (read per call: A/B runs switch them within one process)
static SweepOverrides sweep_overrides() {
  auto opt = [](const char* name) {
    const char* s = std::getenv(name);
    return (s && *s) ? SweepOpt{true, std::atol(s)} : SweepOpt{};
  };
  SweepOverrides o;
  o.reg_streams = opt("AARMVS_REG_STREAMS");
  o.reg_streams_rec = opt("AARMVS_REG_STREAMS_REC");
  o.small_px = opt("AARMVS_SMALL_PX");
  o.npl = opt("AARMVS_NPL");
  o.reg_map = std::getenv("AARMVS_REG_MAP");
  return o;
}

hipError_t aarmvs::library_stream(int dev, int i, hipStream_t& out) {
  static std::mutex mu;
  static hipStream_t pool[kMaxDevices][kLibStreams + 1] = {};
  if (dev < 0 || dev >= kMaxDevices || i < 1 || i > kLibStreams) return hipErrorInvalidValue;
  std::lock_guard<std::mutex> lk(mu);
  if (!pool[dev][i]) {
    hipError_t e = hipStreamCreateWithFlags(&pool[dev][i], hipStreamNonBlocking);
    if (e != hipSuccess) {
      pool[dev][i] = nullptr;
      return e;
    }
  }
  out = pool[dev][i];
  return hipSuccess;
}

// The plane range of a call against the planes its record holds (include/aarmvs.h, "Segment
// records"): record_d0 / record_planes as given (0 planes: up to D).
static int check_record_range(const std::string& who, int D, int d_begin, int d_end, int rec_d0, int rec_n) {
  if (rec_d0 < 0 || rec_n < 0 || rec_d0 >= D || rec_d0 + rec_n > D)
    return fail(AARMVS_ERR_INVALID, who + ": the record's planes (record_d0 " + std::to_string(rec_d0) +
                                        ", record_planes " + std::to_string(rec_n) + ") lie outside [0, D = " +
                                        std::to_string(D) + "]");
  const int rec_end = rec_n ? rec_d0 + rec_n : D;
  if (d_begin < rec_d0 || d_end > rec_end)
    return fail(AARMVS_ERR_INVALID, who + ": the record holds planes [" + std::to_string(rec_d0) + ", " +
                                        std::to_string(rec_end) + ") and does not cover the range [" +
                                        std::to_string(d_begin) + ", " + std::to_string(d_end) + ")");
  return AARMVS_OK;
}

// A segment record addressed as a whole one: every buffer's base moved back by d0 slabs, so that
// plane d's slab sits at index d, as the sweep, the BPTT and the cost-slice backward index it.
// Only the slabs of planes the record holds are ever formed into addresses that are used
// (check_record_range); the moved bases themselves are never dereferenced.
static aarmvs_train_record rebase_record(const aarmvs_train_record& r, const TrainLayout& T, const Workspace& ws,
                                         int d0) {
  aarmvs_train_record v = r;
  if (d0 == 0) return v;
  const ptrdiff_t d = d0;
  v.x = r.x - d * (ptrdiff_t)T.x_plane;
  v.state = r.state - d * (ptrdiff_t)T.state_slab;
  v.z = r.z - d * (ptrdiff_t)T.z_slab;
  v.u = r.u - d * (ptrdiff_t)T.u_slab;
  v.stats = r.stats - d * (ptrdiff_t)T.stats_slab;
  v.t1 = r.t1 - d * (ptrdiff_t)(ws.t1_plane * 4);
  v.ostats = r.ostats - d * (ptrdiff_t)(ws.omega_stats_bytes / sizeof(double));
  return v;
}

// the c8 feature copies of the cost stage; each copy also folds 8 max|feature|^2 into ws.xbound
// (cell 0's fp16 range guard), zeroed first
static int make_feature_copies(const std::string& who, const float* ref, const float* const* src, int nsrc, int B,
                               int HW, const Workspace& ws, hipStream_t stream) {
  hipError_t e;
  if ((e = hipMemsetAsync(ws.xbound, 0, sizeof(unsigned), stream)) != hipSuccess)
    return hip_fail(e, (who + ": bound init").c_str());
  if ((e = launch_to_c8(ref, ws.feat8[0], B, HW, stream, ws.xbound)) != hipSuccess)
    return hip_fail(e, (who + ": c8 copy").c_str());
  for (int v = 0; v < nsrc; ++v)
    if ((e = launch_to_c8(src[v], ws.feat8[1 + v], B, HW, stream, ws.xbound)) != hipSuccess)
      return hip_fail(e, (who + ": c8 copy").c_str());
  return AARMVS_OK;
}

// walk_sweep's sink: one sweep call's launches, event records and event waits on HIP
struct HipSweep {
  const aarmvs_sweep_args* a;
  const TrainLayout& T;
  const SweepGeom& g;
  const Workspace& ws;
  const CostArgs& ca;
  hipEvent_t* ev;
  hipStream_t st[kSweepSlots];
  int precision = AARMVS_PREC_SPLIT;   // aarmvs_precision of the regulariser's units
  void* refine_state = nullptr;        // aarmvs_refine_args.state: the head also keeps it
  void* posterior_state = nullptr;     // aarmvs_posterior_args.state: likewise
  int rc = 0, io_d = -1;
  UnetIO io_{};

  // the call's error is its first failure (the joins still run after one)
  int check(hipError_t e, const char* where) {
    if (e == hipSuccess) return 0;
    if (!rc) rc = hip_fail(e, where);
    return rc;
  }
  // the group's cost slices: two alternating workspace slots, or the record's planes
  float* slices(const SweepGroup& grp) const {
    return a->record ? a->record->x + (size_t)grp.g0 * T.x_plane : ws.xg[grp.gi & 1];
  }
  const float* slice(const SweepGroup& grp, int d) const {
    return slices(grp) + (size_t)(d - grp.g0) * ws.x_plane;
  }
  // plane d's tensors (kept from one unit of the plane to the next); own: the unit stores its
  // statistics, never accumulates them (one writer each)
  const UnetIO& io(int d, bool own) {
    if (d != io_d) io_ = a->record ? unet_io_record(T, *a->record, d) : unet_io_ws(ws, d);
    io_d = d;
    io_.clear_stats = !own && !a->record;
    return io_;
  }

  int fork(int slot, int i) {
    hipError_t e = hipEventRecord(ev[i], st[0]);
    if (e == hipSuccess) e = hipStreamWaitEvent(st[slot], ev[i], 0);
    return check(e, "sweep: fork");
  }
  int join(int slot, int i) {
    if (st[slot] == st[0]) return 0;
    hipError_t e = hipEventRecord(ev[i], st[slot]);
    if (e == hipSuccess) e = hipStreamWaitEvent(st[0], ev[i], 0);
    return check(e, "sweep: join");
  }
  int wait(int slot, int i) { return check(hipStreamWaitEvent(st[slot], ev[i], 0), "sweep: event wait"); }
  int record(int slot, int i) { return check(hipEventRecord(ev[i], st[slot]), "sweep: event record"); }
  int cost_group(int slot, const SweepGroup& grp) {
    const aarmvs_train_record* rec = a->record;
    // training: the group's omega conv output and statistics go straight to the record (the
    // backward reads them instead of recomputing the omega conv; the record's per-plane layout
    // is the workspace slots')
    Workspace wsg = ws;
    if (rec) {
      wsg.t1 = rec->t1 + (size_t)grp.g0 * ws.t1_plane * 4;
      wsg.omega_stats = rec->ostats + (size_t)grp.g0 * (ws.omega_stats_bytes / 8);
    }
    if (int r = check(launch_omega_group(ca, g, wsg, grp.g0, grp.n, st[slot], rec != nullptr), "sweep: omega stage"))
      return r;
    const int d_last = a->d_end - 1, ok = d_last < grp.g0 + grp.n ? d_last - grp.g0 : -1;
    return check(launch_cost_x_group(ca, g, wsg, grp.g0, grp.n, slices(grp), ok >= 0 ? a->omega_out : nullptr,
                                     ok, st[slot]),
                 "sweep: cost slices");
  }
  int slice_copy(const SweepGroup& grp, int d) {
    return check(launch_layout(slice(grp, d), a->slice_out, a->B, kC, a->H * a->W, false, st[0]),
                 "sweep: slice copy");
  }
  int step(const SweepGroup& grp, int d) {
    const UnetIO& all = io(d, false);
    if (int r = check(launch_unet_step(slice(grp, d), ca.params, g, ws, all, st[0], kUnetAll, precision),
                      "sweep: regulariser step"))
      return r;
    return head_on(st[0], all, d);
  }
  int unit(int slot, int u, const SweepGroup& grp, int d) {
    return check(launch_unet_step(slice(grp, d), ca.params, g, ws, io(d, true), st[slot], 1 << u, precision),
                 "sweep: regulariser step");
  }
  int head(int slot, int d) { return head_on(st[slot], io(d, true), d); }
  // the WTA images are maintained on every plane, whether or not this call returns depth:
  // a sweep split into d_range calls gives the same depth/confidence however its earlier
  // pieces were requested (24 B/px per plane, <0.5% of a plane's time)
  int head_on(hipStream_t s, const UnetIO& io, int d) {
    return check(launch_head_wta(ca.params, g, io, ws, a->depth_values, d, a->cost_out, true, s, refine_state,
                                 posterior_state),
                 "sweep: head/wta");
  }
};

extern "C" {

int aarmvs_sweep(const aarmvs_sweep_args* a, hipStream_t stream) {
  return aarmvs_sweep_p(a, AARMVS_PREC_SPLIT, stream);
}

int aarmvs_sweep_p(const aarmvs_sweep_args* a, int precision, hipStream_t stream) {
  return aarmvs_sweep_r(a, precision, nullptr, stream);
}

int aarmvs_sweep_r(const aarmvs_sweep_args* a, int precision, const aarmvs_refine_args* refine,
                   hipStream_t stream) {
  aarmvs_sweep_options o{};
  o.size = sizeof(o);
  o.precision = precision;
  o.refine = refine;
  return aarmvs_sweep_ex(a, &o, stream);
}

size_t aarmvs_posterior_state_bytes(int B, int HW) {
  if (B < 1 || HW < 1) return 0;
  return (size_t)16 * B * HW;
}

size_t aarmvs_refine_state_bytes(int B, int HW) {
  if (B < 1 || HW < 1) return 0;
  return (size_t)16 * B * HW;
}

int aarmvs_sweep_ex(const aarmvs_sweep_args* a, const aarmvs_sweep_options* options,
                    hipStream_t stream) {
  if (!a) return fail(AARMVS_ERR_INVALID, "sweep: null args");
  // the caller's struct may be older (shorter) than the library's: fields beyond its size are zero
  aarmvs_sweep_options o{};
  if (options) {
    if (options->size < AARMVS_SWEEP_OPTIONS_SIZE_V1 || options->size > sizeof(o))
      return fail(AARMVS_ERR_INVALID,
                  "sweep: aarmvs_sweep_options.size " + std::to_string(options->size) + " outside [" +
                      std::to_string(AARMVS_SWEEP_OPTIONS_SIZE_V1) + ", " + std::to_string(sizeof(o)) +
                      "] (set it to sizeof(aarmvs_sweep_options))");
    std::memcpy(&o, options, options->size);
  }
  const int precision = o.precision;
  const aarmvs_refine_args* refine = o.refine;
  const aarmvs_posterior_args* posterior = o.posterior;
  if (posterior && !posterior->state)
    return fail(AARMVS_ERR_INVALID, "sweep: aarmvs_posterior_args without a state buffer "
                                    "(aarmvs_posterior_state_bytes(B, H * W) bytes of device memory)");
  if (posterior && a->record)
    return fail(AARMVS_ERR_INVALID,
                "sweep: the depth-posterior statistics are an inference output; a recorded (training) "
                "sweep takes no aarmvs_posterior_args (aarmvs_posterior_from_cost works on its cost volume)");
  if (refine && !refine->state)
    return fail(AARMVS_ERR_INVALID, "sweep: aarmvs_refine_args without a state buffer "
                                    "(aarmvs_refine_state_bytes(B, H * W) bytes of device memory)");
  if (refine && a->record)
    return fail(AARMVS_ERR_INVALID,
                "sweep: the sub-plane refinement is an inference output; a recorded (training) sweep "
                "takes no aarmvs_refine_args (aarmvs_refine_from_cost works on its cost volume)");
  if (precision != AARMVS_PREC_SPLIT && precision != AARMVS_PREC_FP16)
    return fail(AARMVS_ERR_INVALID, "sweep: unknown precision " + std::to_string(precision) +
                                        " (AARMVS_PREC_SPLIT = 0, AARMVS_PREC_FP16 = 1)");
  if (precision == AARMVS_PREC_FP16 && a->record)
    return fail(AARMVS_ERR_INVALID,
                "sweep: AARMVS_PREC_FP16 is an inference mode; a training record needs AARMVS_PREC_SPLIT "
                "(the backward differentiates the split cells)");
  int rc = check_geom(a->B, a->H, a->W, a->nsrc);
  if (rc) return rc;
  if (a->C != kC) return fail(AARMVS_ERR_INVALID, "sweep: feature channels C must be 32");
  if (a->D < 1 || a->d_begin < 0 || a->d_end > a->D || a->d_begin >= a->d_end)
    return fail(AARMVS_ERR_INVALID, "sweep: need 0 <= d_begin < d_end <= D");
  if (!a->ref_fea || !a->rel_proj || !a->depth_values || !a->packed_params || !a->workspace)
    return fail(AARMVS_ERR_INVALID, "sweep: null pointer argument");
  for (int v = 0; v < a->nsrc; ++v)
    if (!a->src_fea[v]) return fail(AARMVS_ERR_INVALID, "sweep: null src_fea pointer");
  const aarmvs_train_record* rec = a->record;
  if (rec && (!rec->x || !rec->state || !rec->z || !rec->u || !rec->stats || !rec->t1 || !rec->ostats))
    return fail(AARMVS_ERR_INVALID, "sweep: training record with a null buffer");
  if (rec && (rc = check_record_range("sweep", a->D, a->d_begin, a->d_end, a->record_d0, a->record_planes)))
    return rc;
  const TrainLayout T = train_layout(a->B, a->H, a->W);

  SweepGeom g{a->B, a->H, a->W, a->nsrc, a->D, cu_count()};
  Workspace ws = carve_workspace(a->workspace, a->B, a->H, a->W, a->nsrc);
  // a segment record is addressed by the absolute plane from here on
  aarmvs_train_record rec_abs{};
  aarmvs_sweep_args a_abs = *a;
  if (rec) {
    rec_abs = rebase_record(*rec, T, ws, a->record_d0);
    a_abs.record = rec = &rec_abs;
    a = &a_abs;
  }
  const float* params = static_cast<const float*>(a->packed_params);
  hipError_t e;
  CostArgs ca{};
  ca.ref = a->ref_fea;
  for (int v = 0; v < a->nsrc; ++v) ca.src[v] = a->src_fea[v];
  ca.rel = a->rel_proj;
  ca.depth_values = a->depth_values;
  ca.params = params;
  // under stream capture (a caller recording the sweep into a graph) everything stays on `stream`
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if ((e = hipStreamIsCapturing(stream, &cap)) != hipSuccess) return hip_fail(e, "sweep: capture status");
  const SweepPlan plan =
      plan_sweep(a->aux_stream && a->aux_stream != stream, cap != hipStreamCaptureStatusNone, rec != nullptr,
                 (long)a->B * a->H * a->W, sweep_overrides());
  // The events: a per-thread, per-device set reused across calls (a sweep split into d_range
  // pieces makes one call per piece).  Events are only recorded/waited on the caller's streams and the set's
  // own, and a record overwrites the previous one, so reuse is safe.
  struct EventSet {
    int dev = -1;
    hipEvent_t ev[kSweepEvents] = {};
  };
  static thread_local EventSet evs_dev[kMaxDevices];   // one set per device
  int dev = 0;
  if ((e = current_device(dev)) != hipSuccess) return hip_fail(e, "sweep: get device");
  EventSet& evs = evs_dev[dev];
  if (plan.events() && evs.dev != dev) {
    for (hipEvent_t& x : evs.ev)
      if ((e = hipEventCreateWithFlags(&x, hipEventDisableTiming)) != hipSuccess)
        return hip_fail(e, "sweep: event create");
    evs.dev = dev;
  }
  HipSweep run{a, T, g, ws, ca, evs.ev, {}};
  run.precision = precision;
  run.refine_state = refine ? refine->state : nullptr;
  run.posterior_state = posterior ? posterior->state : nullptr;
  for (int i = 0; i < kSweepSlots; ++i) {
    const SweepStream id = plan.slot[i];
    if (id == kCaller) run.st[i] = stream;
    if (id == kCallerAux) run.st[i] = a->aux_stream;
    if (id >= kLib1 && (e = library_stream(dev, id - kLib1 + 1, run.st[i])) != hipSuccess)
      return hip_fail(e, "sweep: stream create");
  }

  if (a->d_begin == 0) {
    // UNetConvLSTM._init_hidden (drmvsnet.py:133-134, 202-206) and the WTA images
    // (drmvsnet.py:302-304)
    if ((e = hipMemsetAsync(ws.state_begin, 0, ws.state_bytes, stream)) != hipSuccess)
      return hip_fail(e, "sweep: state init");
    if ((e = hipMemsetAsync(ws.max_prob, 0, ws.wta_bytes, stream)) != hipSuccess)
      return hip_fail(e, "sweep: wta init");
    if ((e = hipMemsetAsync(ws.omega_stats, 0, ws.stats_bytes, stream)) != hipSuccess)
      return hip_fail(e, "sweep: stats init");
    if (rec && (e = hipMemsetAsync(rec->state, 0, T.state_slab * sizeof(float), stream)) != hipSuccess)
      return hip_fail(e, "sweep: record state init");
    // c8 copies of the features for the cost stage
    const int HW = a->H * a->W;
    // (each copy also folds 8 max|feature|^2 into ws.xbound: cell 0's fp16 range guard)
    if ((e = launch_to_c8(a->ref_fea, ws.feat8[0], a->B, HW, stream, ws.xbound)) != hipSuccess)
      return hip_fail(e, "sweep: c8 copy");
    for (int v = 0; v < a->nsrc; ++v)
      if ((e = launch_to_c8(a->src_fea[v], ws.feat8[1 + v], a->B, HW, stream, ws.xbound)) !=
          hipSuccess)
        return hip_fail(e, "sweep: c8 copy");
  } else if (rec) {
    // A recorded call that starts inside the sweep (a later d_range piece, or the recompute of a
    // checkpointed segment) stands on its own: of what the d_begin == 0 branch prepares, record
    // mode reads the state from the record (slab d_begin - record_d0, the caller's), takes its
    // statistics in the record (zeroed below and per group in launch_omega_group) and needs the
    // WTA images only for depth_out / conf_out; what is left are the c8 feature copies and the
    // guard bound, re-made here as aarmvs_sweep_backward does (the workspace may have served
    // another sweep since; the same values when it has not)
    if ((rc = make_feature_copies("sweep", a->ref_fea, a->src_fea, a->nsrc, a->B, a->H * a->W, ws, stream)))
      return rc;
  }
  // a record's statistics slabs accumulate from zero (block 0 of cells 3 and 4 fills slot 0 of each)
  if (rec && (e = hipMemsetAsync(rec->stats + (size_t)a->d_begin * T.stats_slab, 0,
                                 (size_t)(a->d_end - a->d_begin) * T.stats_slab * sizeof(double),
                                 stream)) != hipSuccess)
    return hip_fail(e, "sweep: record stats init");
  // forks, the groups' cost stages and regulariser steps, joins (sweep_schedule.h)
  if ((rc = walk_sweep(plan, a->d_begin, a->d_end, a->slice_out ? a->d_end - 1 : -1, run))) return rc;
  if ((a->depth_out || a->conf_out) && a->d_end == a->D) {
    if ((e = launch_finalize(g, ws, a->depth_out, a->conf_out, stream)) != hipSuccess)
      return hip_fail(e, "sweep: finalize");
  }
  // the refined outputs describe the planes [0, d_end) of every call (a pixel whose winner is
  // the call's last plane is unrefined until the next call has seen the plane after it)
  if (refine && (refine->depth_refined_out || refine->conf_window_out || refine->index_out)) {
    if ((e = launch_refine_finalize(ws.max_prob, ws.exp_sum, ws.depth, refine->state, a->depth_values,
                                    a->B, a->D, a->d_end, a->H * a->W, refine->depth_refined_out,
                                    refine->conf_window_out, refine->index_out, stream)) != hipSuccess)
      return hip_fail(e, "sweep: refine finalize");
  }
  // likewise the posterior statistics of the planes [0, d_end)
  if (posterior && (posterior->mean_out || posterior->std_out || posterior->entropy_out ||
                    posterior->runner_up_out)) {
    if ((e = launch_posterior_finalize(ws.exp_sum, posterior->state, a->B, a->H * a->W, posterior->mean_out,
                                       posterior->std_out, posterior->entropy_out,
                                       posterior->runner_up_out, stream)) != hipSuccess)
      return hip_fail(e, "sweep: posterior finalize");
  }
  return AARMVS_OK;
}

size_t aarmvs_backward_scratch_bytes(int B, int H, int W, int nsrc) {
  if (check_geom(B, H, W, nsrc) != AARMVS_OK) return 0;
  return bptt_scratch_bytes(B, H, W) + cost_bwd_scratch_bytes(B, H, W, nsrc);
}

int aarmvs_sweep_backward(const aarmvs_backward_args* a, hipStream_t stream) {
  if (!a) return fail(AARMVS_ERR_INVALID, "sweep_backward: null args");
  int rc = check_geom(a->B, a->H, a->W, a->nsrc);
  if (rc) return rc;
  if (a->C != kC) return fail(AARMVS_ERR_INVALID, "sweep_backward: feature channels C must be 32");
  if (a->D < 1 || !a->ref_fea || !a->rel_proj || !a->depth_values || !a->packed_params ||
      !a->record || !a->grad_cost || !a->workspace || !a->scratch)
    return fail(AARMVS_ERR_INVALID, "sweep_backward: null pointer argument or D < 1");
  const aarmvs_train_record* rec = a->record;
  if (!rec->x || !rec->state || !rec->z || !rec->u || !rec->stats || !rec->t1 || !rec->ostats)
    return fail(AARMVS_ERR_INVALID, "sweep_backward: training record with a null buffer");
  for (int v = 0; v < a->nsrc; ++v)
    if (!a->src_fea[v]) return fail(AARMVS_ERR_INVALID, "sweep_backward: null src_fea pointer");
  // (written by the call that ends a backward, d_begin == 0; the earlier calls of a ranged one
  // do not touch the outputs)
  if (!a->regulariser_only && !a->grad_ref && a->d_begin == 0)
    return fail(AARMVS_ERR_INVALID, "sweep_backward: grad_ref is required (the cost-slice part)");
  // the plane range of this call (all zero: the whole backward)
  const int d_begin = a->d_begin, d_end = a->d_end ? a->d_end : a->D;
  if (d_begin < 0 || d_end > a->D || d_begin >= d_end)
    return fail(AARMVS_ERR_INVALID, "sweep_backward: the range [" + std::to_string(d_begin) + ", " +
                                        std::to_string(d_end) + ") lies outside [0, D = " + std::to_string(a->D) +
                                        "] or is empty (need 0 <= d_begin < d_end <= D)");
  if (d_begin % kPlaneGroup || (d_end % kPlaneGroup && d_end != a->D))
    return fail(AARMVS_ERR_INVALID, "sweep_backward: misaligned range [" + std::to_string(d_begin) + ", " +
                                        std::to_string(d_end) + "): d_begin and d_end must be multiples of " +
                                        std::to_string(kPlaneGroup) + " (d_end may equal D), so that the groups "
                                        "are the whole backward's");
  if ((rc = check_record_range("sweep_backward", a->D, d_begin, d_end, a->record_d0, a->record_planes))) return rc;
  Workspace ws = carve_workspace(a->workspace, a->B, a->H, a->W, a->nsrc);
  hipError_t e;
  // a segment record is addressed by the absolute plane from here on
  const aarmvs_train_record rec_abs = rebase_record(*rec, train_layout(a->B, a->H, a->W), ws, a->record_d0);
  aarmvs_backward_args a_abs = *a;
  a_abs.record = rec = &rec_abs;
  a = &a_abs;
  // the c8 feature copies and the fp16 guard bound of the forward, recomputed (the workspace
  // may have served another sweep since)
  if ((rc = make_feature_copies("sweep_backward", a->ref_fea, a->src_fea, a->nsrc, a->B, a->H * a->W, ws, stream)))
    return rc;
  char* scratch = static_cast<char*>(a->scratch);
  const size_t breg = bptt_scratch_bytes(a->B, a->H, a->W);
  CostBwdCtx cctx{};
  cctx.a = a;
  cctx.ws = ws;
  cctx.scratch = scratch + breg;
  cctx.gacc = bptt_gacc(scratch, a->B, a->H, a->W);
  // the first call of a backward (its last planes) zeroes what the calls carry in `scratch`
  // (here the cost-slice accumulators, in bptt_regulariser the state gradients and gacc), the
  // last one (d_begin == 0) folds them into the outputs
  if (!a->regulariser_only && d_end == a->D && (e = cost_bwd_begin(cctx, stream)) != hipSuccess)
    return hip_fail(e, "sweep_backward: cost-slice init");
  BpttRun r{};
  r.B = a->B;
  r.H = a->H;
  r.W = a->W;
  r.D = a->D;
  r.d_begin = d_begin;
  r.d_end = d_end;
  r.packed = static_cast<const float*>(a->packed_params);
  r.rec = rec;
  r.grad_cost = a->grad_cost;
  r.xbound = ws.xbound;
  r.scratch = scratch;
  r.grad_x = a->grad_x;
  r.grad_params = a->grad_params;
  r.group_done = a->regulariser_only ? nullptr : cost_bwd_group;
  r.ctx = &cctx;
  if ((e = bptt_regulariser(r, stream)) != hipSuccess) return hip_fail(e, "sweep_backward");
  if (!a->regulariser_only && d_begin == 0 && (e = cost_bwd_end(cctx, stream)) != hipSuccess)
    return hip_fail(e, "sweep_backward: cost-slice gradients");
  return AARMVS_OK;
}

int aarmvs_cost_slice(const float* ref_fea, const float* const* src_fea, const float* rel_proj,
                      const float* depth_d, const void* packed_params, int B, int C, int H, int W,
                      int nsrc, void* workspace, float* slice_out, float* omega_out,
                      hipStream_t stream) {
  int rc = check_geom(B, H, W, nsrc);
  if (rc) return rc;
  if (C != kC) return fail(AARMVS_ERR_INVALID, "cost_slice: feature channels C must be 32");
  if (!ref_fea || !src_fea || !rel_proj || !depth_d || !packed_params || !workspace || !slice_out)
    return fail(AARMVS_ERR_INVALID, "cost_slice: null pointer argument");
  for (int v = 0; v < nsrc; ++v)
    if (!src_fea[v]) return fail(AARMVS_ERR_INVALID, "cost_slice: null src_fea pointer");
  // one plane of the sweep's cost-slice pipeline (D = 1, depth_values = depth_d [B,1])
  SweepGeom g{B, H, W, nsrc, 1, cu_count()};
  Workspace ws = carve_workspace(workspace, B, H, W, nsrc);
  CostArgs ca{};
  ca.ref = ref_fea;
  for (int v = 0; v < nsrc; ++v) ca.src[v] = src_fea[v];
  ca.rel = rel_proj;
  ca.depth_values = depth_d;
  ca.params = static_cast<const float*>(packed_params);
  hipError_t e;
  const int HW = H * W;
  if ((e = hipMemsetAsync(ws.xbound, 0, sizeof(unsigned), stream)) != hipSuccess)
    return hip_fail(e, "cost_slice: bound init");
  if ((e = launch_to_c8(ref_fea, ws.feat8[0], B, HW, stream, ws.xbound)) != hipSuccess)
    return hip_fail(e, "cost_slice: c8 copy");
  for (int v = 0; v < nsrc; ++v)
    if ((e = launch_to_c8(src_fea[v], ws.feat8[1 + v], B, HW, stream, ws.xbound)) != hipSuccess)
      return hip_fail(e, "cost_slice: c8 copy");
  if ((e = launch_omega_group(ca, g, ws, 0, 1, stream)) != hipSuccess)
    return hip_fail(e, "cost_slice: omega stage");
  if ((e = launch_cost_x_group(ca, g, ws, 0, 1, ws.x, omega_out, 0, stream)) != hipSuccess)
    return hip_fail(e, "cost_slice: cost slice");
  if ((e = launch_layout(ws.x, slice_out, B, kC, HW, false, stream)) != hipSuccess)
    return hip_fail(e, "cost_slice: slice copy");
  return AARMVS_OK;
}

int aarmvs_wta_update(const float* cost, const float* depth_d, float* max_prob, float* depth_map,
                      float* exp_sum, int B, int HW, hipStream_t stream) {
  if (!cost || !depth_d || !max_prob || !depth_map || !exp_sum || B < 1 || HW < 1)
    return fail(AARMVS_ERR_INVALID, "wta_update: bad arguments");
  hipError_t e = launch_wta_update(cost, depth_d, max_prob, depth_map, exp_sum, B, HW, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "wta_update");
}

int aarmvs_wta_refine_update(const float* cost, int d, float* max_prob, float* depth_map,
                             float* exp_sum, void* state, const float* depth_d, int B, int HW,
                             hipStream_t stream) {
  if (!cost || !depth_d || !max_prob || !depth_map || !exp_sum || !state || B < 1 || HW < 1 || d < 0)
    return fail(AARMVS_ERR_INVALID, "wta_refine_update: bad arguments");
  hipError_t e = launch_wta_refine_update(cost, depth_d, d, max_prob, depth_map, exp_sum, state, B, HW, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "wta_refine_update");
}

int aarmvs_wta_refine_finalize(const float* max_prob, const float* depth_map, const float* exp_sum,
                               const void* state, const float* depth_values, int B, int D, int n,
                               int HW, float* depth_refined, float* conf_window, int* index,
                               hipStream_t stream) {
  if (!max_prob || !depth_map || !exp_sum || !state || !depth_values)
    return fail(AARMVS_ERR_INVALID, "wta_refine_finalize: null pointer argument");
  if (B < 1 || HW < 1 || D < 1 || n < 1 || n > D)
    return fail(AARMVS_ERR_INVALID, "wta_refine_finalize: need B, HW >= 1 and 1 <= n <= D");
  hipError_t e = launch_refine_finalize(max_prob, exp_sum, depth_map, state, depth_values, B, D, n, HW,
                                        depth_refined, conf_window, index, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "wta_refine_finalize");
}

int aarmvs_refine_from_cost(const float* cost, const float* depth_values, int B, int D, int HW,
                            float* depth_refined, float* conf_window, int* index, hipStream_t stream) {
  if (!cost || !depth_values)
    return fail(AARMVS_ERR_INVALID, "refine_from_cost: null pointer argument");
  if (B < 1 || D < 1 || HW < 1)
    return fail(AARMVS_ERR_INVALID, "refine_from_cost: need B, D, HW >= 1");
  hipError_t e = launch_refine_from_cost(cost, depth_values, B, D, HW, depth_refined, conf_window, index, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "refine_from_cost");
}

int aarmvs_wta_posterior_update(const float* cost, int d, float* max_prob, float* depth_map,
                                float* exp_sum, void* state, const float* depth_d, int B, int HW,
                                hipStream_t stream) {
  if (!cost || !depth_d || !max_prob || !depth_map || !exp_sum || !state || B < 1 || HW < 1 || d < 0)
    return fail(AARMVS_ERR_INVALID, "wta_posterior_update: bad arguments");
  hipError_t e = launch_wta_posterior_update(cost, depth_d, d, max_prob, depth_map, exp_sum, state, B, HW, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "wta_posterior_update");
}

int aarmvs_wta_posterior_finalize(const float* exp_sum, const void* state, int B, int HW, float* mean,
                                  float* std_out, float* entropy, float* runner_up, hipStream_t stream) {
  if (!exp_sum || !state) return fail(AARMVS_ERR_INVALID, "wta_posterior_finalize: null pointer argument");
  if (B < 1 || HW < 1) return fail(AARMVS_ERR_INVALID, "wta_posterior_finalize: need B, HW >= 1");
  hipError_t e = launch_posterior_finalize(exp_sum, state, B, HW, mean, std_out, entropy, runner_up, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "wta_posterior_finalize");
}

int aarmvs_posterior_from_cost(const float* cost, const float* depth_values, int B, int D, int HW,
                               float* mean, float* std_out, float* entropy, float* runner_up,
                               hipStream_t stream) {
  if (!cost || !depth_values)
    return fail(AARMVS_ERR_INVALID, "posterior_from_cost: null pointer argument");
  if (B < 1 || D < 1 || HW < 1)
    return fail(AARMVS_ERR_INVALID, "posterior_from_cost: need B, D, HW >= 1");
  hipError_t e = launch_posterior_from_cost(cost, depth_values, B, D, HW, mean, std_out, entropy, runner_up, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "posterior_from_cost");
}

int aarmvs_unet_step(const float* x, int B, int H, int W, int nsrc, int step,
                     const void* packed_params, void* workspace, float* cost_out,
                     hipStream_t stream) {
  return aarmvs_unet_step_p(x, B, H, W, nsrc, step, packed_params, workspace, cost_out, AARMVS_PREC_SPLIT, stream);
}

int aarmvs_unet_step_p(const float* x, int B, int H, int W, int nsrc, int step,
                       const void* packed_params, void* workspace, float* cost_out, int precision,
                       hipStream_t stream) {
  if (precision != AARMVS_PREC_SPLIT && precision != AARMVS_PREC_FP16)
    return fail(AARMVS_ERR_INVALID, "unet_step: unknown precision " + std::to_string(precision) +
                                        " (AARMVS_PREC_SPLIT = 0, AARMVS_PREC_FP16 = 1)");
  int rc = check_geom(B, H, W, nsrc);
  if (rc) return rc;
  if (!x || !packed_params || !workspace || !cost_out || step < 0)
    return fail(AARMVS_ERR_INVALID, "unet_step: null pointer or negative step");
  SweepGeom g{B, H, W, nsrc, 1, cu_count()};
  Workspace ws = carve_workspace(workspace, B, H, W, nsrc);
  const float* params = static_cast<const float*>(packed_params);
  hipError_t e;
  if (step == 0 && (e = hipMemsetAsync(ws.state_begin, 0, ws.state_bytes, stream)) != hipSuccess)
    return hip_fail(e, "unet_step: state init");
  if ((e = hipMemsetAsync(ws.reg_stats, 0, ws.reg_stats_bytes, stream)) != hipSuccess)
    return hip_fail(e, "unet_step: stats reset");
  // the workspace's slice buffer holds x as NHWC, like the sweep's cost slice; max|x| goes
  // to ws.xbound (cell 0's fp16 range guard)
  if ((e = hipMemsetAsync(ws.xbound, 0, sizeof(unsigned), stream)) != hipSuccess)
    return hip_fail(e, "unet_step: bound reset");
  if ((e = launch_layout(x, ws.x, B, kC, H * W, true, stream, ws.xbound)) != hipSuccess)
    return hip_fail(e, "unet_step: x layout");
  const UnetIO io = unet_io_ws(ws, step);
  if ((e = launch_unet_step(ws.x, params, g, ws, io, stream, kUnetAll, precision)) != hipSuccess)
    return hip_fail(e, "unet_step");
  // head conv only (no WTA): cost_out is [B,1,H,W] == [B,D=1,H,W] at plane 0
  if ((e = launch_head_wta(params, g, io, ws, nullptr, 0, cost_out, false, stream)) !=
      hipSuccess)
    return hip_fail(e, "unet_step: head");
  return AARMVS_OK;
}

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
  hipError_t e = launch_fusion_filter(a, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "fusion_filter");
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
  hipError_t e = launch_fusion_filter_dedup(a, d, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "fusion_filter_dedup");
}

int aarmvs_pyr_down(const float* src, int H, int W, int C, float* dst, hipStream_t stream) {
  if (!src || !dst) return fail(AARMVS_ERR_INVALID, "pyr_down: null pointer argument");
  if (H < 4 || W < 4 || (C != 1 && C != 3))
    return fail(AARMVS_ERR_INVALID, "pyr_down: need H, W >= 4 and C = 1 or 3");
  if ((long long)H * W * C >= (1LL << 31))
    return fail(AARMVS_ERR_INVALID, "pyr_down: H * W * C must be below 2^31");
  hipError_t e = launch_pyr_down(src, H, W, C, dst, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "pyr_down");
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
  hipError_t e = launch_fusion_points(a, nullptr, nullptr, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "fusion_points");
}

int aarmvs_fusion_points_normals(const aarmvs_fusion_points_args* a, const float* normal_map, float* nxyz,
                                 hipStream_t stream) {
  if (!normal_map && !nxyz) return aarmvs_fusion_points(a, stream);
  if (int rc = fusion_points_check(a)) return rc;
  if (!normal_map || !nxyz)
    return fail(AARMVS_ERR_INVALID,
                "fusion_points_normals: normal_map and nxyz must both be set or both be null");
  hipError_t e = launch_fusion_points(a, normal_map, nxyz, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "fusion_points_normals");
}

// [p, p + n) and [q, q + m) share a byte
static bool ranges_overlap(const void* p, size_t n, const void* q, size_t m) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + m && b < a + n;
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
  hipError_t e = launch_fusion_normals(a, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "fusion_normals");
}

size_t aarmvs_group_norm_scratch_bytes(int B, int C, int HW) {
  return (B < 1 || C < 1 || HW < 1) ? 0 : gn_scratch_bytes(B, C, HW);
}

int aarmvs_group_norm_forward(const float* x, const float* gamma, const float* beta, int B, int C,
                              int HW, int G, float eps, float* y, float* mean_rstd, void* scratch,
                              hipStream_t stream) {
  if (!x || !y || !mean_rstd || !scratch || B < 1 || C < 1 || HW < 1 || G < 1 || C % G != 0 ||
      B > 65535 || C > 65535)
    return fail(AARMVS_ERR_INVALID, "group_norm_forward: bad arguments (need G | C)");
  hipError_t e = launch_group_norm_fwd(x, gamma, beta, B, C, HW, G, eps, y, mean_rstd, scratch, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "group_norm_forward");
}

int aarmvs_group_norm_backward(const float* dy, const float* x, const float* gamma,
                               const float* mean_rstd, int B, int C, int HW, int G, float* dx,
                               float* s1, float* s2, void* scratch, hipStream_t stream) {
  if (!dy || !x || !mean_rstd || !dx || !s1 || !s2 || !scratch || B < 1 || C < 1 || HW < 1 ||
      G < 1 || C % G != 0 || B > 65535 || C > 65535)
    return fail(AARMVS_ERR_INVALID, "group_norm_backward: bad arguments (need G | C)");
  hipError_t e = launch_group_norm_bwd(dy, x, gamma, mean_rstd, B, C, HW, G, dx, s1, s2, scratch, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "group_norm_backward");
}

int aarmvs_lstm_gates_forward(const float* z, const float* c_prev, int B, int hid, int HW, float* h,
                              float* c, hipStream_t stream) {
  if (!z || !c_prev || !h || !c || B < 1 || hid < 1 || HW < 1)
    return fail(AARMVS_ERR_INVALID, "lstm_gates_forward: bad arguments");
  hipError_t e = launch_lstm_gates_fwd(z, c_prev, B, hid, HW, h, c, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "lstm_gates_forward");
}

int aarmvs_lstm_gates_backward(const float* z, const float* c_prev, const float* dh, const float* dc,
                               int B, int hid, int HW, float* dz, float* dc_prev, hipStream_t stream) {
  if (!z || !c_prev || !dz || !dc_prev || B < 1 || hid < 1 || HW < 1)
    return fail(AARMVS_ERR_INVALID, "lstm_gates_backward: bad arguments");
  hipError_t e = launch_lstm_gates_bwd(z, c_prev, dh, dc, B, hid, HW, dz, dc_prev, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "lstm_gates_backward");
}

int aarmvs_softmax_depth(const float* cost, float* prob, int B, int D, int HW, hipStream_t stream) {
  if (!cost || !prob || B < 1 || D < 1 || HW < 1)
    return fail(AARMVS_ERR_INVALID, "softmax_depth: bad arguments");
  hipError_t e = launch_softmax_depth(cost, prob, B, D, HW, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "softmax_depth");
}

int aarmvs_evidential_epilogue(const float* const head[3], const float* depth_values, int D, int HW,
                               float* evidential, float* prob_combine, hipStream_t stream) {
  if (!head || !head[0] || !head[1] || !head[2] || !depth_values || !evidential || !prob_combine ||
      HW < 1)
    return fail(AARMVS_ERR_INVALID, "evidential_epilogue: null pointer or HW < 1");
  if (D != AARMVS_EVIDENTIAL_D)
    return fail(AARMVS_ERR_INVALID, "evidential_epilogue: D must be 32 (the head's maxdisp)");
  hipError_t e = launch_evidential(head, depth_values, D, HW, evidential, prob_combine, nullptr,
                                   nullptr, nullptr, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "evidential_epilogue");
}

int aarmvs_evidential_epilogue_backward(const float* const head[3], const float* depth_values, int D,
                                        int HW, const float* grad_evidential,
                                        const float* grad_prob_combine, float* const grad_head[3],
                                        hipStream_t stream) {
  if (!head || !head[0] || !head[1] || !head[2] || !depth_values || !grad_head || !grad_head[0] ||
      !grad_head[1] || !grad_head[2] || HW < 1)
    return fail(AARMVS_ERR_INVALID, "evidential_epilogue_backward: null pointer or HW < 1");
  if (D != AARMVS_EVIDENTIAL_D)
    return fail(AARMVS_ERR_INVALID, "evidential_epilogue_backward: D must be 32 (the head's maxdisp)");
  hipError_t e = launch_evidential(head, depth_values, D, HW, nullptr, nullptr, grad_evidential,
                                   grad_prob_combine, grad_head, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "evidential_epilogue_backward");
}

static int deform_check(const char* who, const float* x, const float* offset, int B, int C, int H,
                        int W, int h, int w, int stride, int pad) {
  if (!x || !offset) return fail(AARMVS_ERR_INVALID, std::string(who) + ": null pointer");
  if (C != AARMVS_DEFORM_C)
    return fail(AARMVS_ERR_INVALID, std::string(who) + ": C must be 32 (FeatNet's deformable convs)");
  if (B < 1 || H < 1 || W < 1 || h < 1 || w < 1 || stride < 1 || pad < 0)
    return fail(AARMVS_ERR_INVALID, std::string(who) + ": bad geometry");
  return AARMVS_OK;
}

static DfArgs deform_args(const float* x, const float* offset, const float* mask, int B, int H,
                          int W, int h, int w, int stride, int pad) {
  DfArgs a{};
  a.x = x;
  a.off = offset;
  a.m = mask;
  a.B = B;
  a.H = H;
  a.W = W;
  a.h = h;
  a.w = w;
  a.stride = stride;
  a.pad = pad;
  return a;
}

int aarmvs_deform_sample(const float* x_nhwc, const float* offset, const float* mask, int B, int C,
                         int H, int W, int h, int w, int stride, int pad, float* val,
                         hipStream_t stream) {
  if (int rc = deform_check("deform_sample", x_nhwc, offset, B, C, H, W, h, w, stride, pad)) return rc;
  if (!val) return fail(AARMVS_ERR_INVALID, "deform_sample: null pointer");
  DfArgs a = deform_args(x_nhwc, offset, mask, B, H, W, h, w, stride, pad);
  a.val = val;
  hipError_t e = launch_deform_sample(a, false, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "deform_sample");
}

int aarmvs_deform_sample_backward(const float* x_nhwc, const float* offset, const float* mask, int B,
                                  int C, int H, int W, int h, int w, int stride, int pad,
                                  const float* grad_val, float* grad_x_nhwc, float* grad_offset,
                                  float* grad_mask, hipStream_t stream) {
  if (int rc = deform_check("deform_sample_backward", x_nhwc, offset, B, C, H, W, h, w, stride, pad))
    return rc;
  if (!grad_val || !grad_x_nhwc || !grad_offset || (mask && !grad_mask))
    return fail(AARMVS_ERR_INVALID, "deform_sample_backward: null pointer");
  DfArgs a = deform_args(x_nhwc, offset, mask, B, H, W, h, w, stride, pad);
  a.gval = grad_val;
  a.gx = grad_x_nhwc;
  a.goff = grad_offset;
  a.gm = mask ? grad_mask : nullptr;
  hipError_t e = launch_deform_sample(a, true, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "deform_sample_backward");
}

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
  hipError_t e = launch_cls_loss_fwd(cost, depth_gt, mask, depth_values, B, D, HW, loss, wta_depth,
                                     max_prob, lse, gt_index, coef, scratch, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "cls_loss");
}

int aarmvs_cls_loss_backward(const float* cost, const float* lse, const int* gt_index,
                             const float* mask, const float* coef, const float* grad_loss, int B,
                             int D, int HW, float* grad_cost, hipStream_t stream) {
  if (!cost || !lse || !gt_index || !mask || !coef || !grad_loss || !grad_cost)
    return fail(AARMVS_ERR_INVALID, "cls_loss_backward: null pointer argument");
  if (int rc = cls_check("cls_loss_backward", B, HW)) return rc;
  if (D < 1) return fail(AARMVS_ERR_INVALID, "cls_loss_backward: need D >= 1");
  hipError_t e = launch_cls_loss_bwd(cost, lse, gt_index, mask, coef, grad_loss, B, D, HW, grad_cost,
                                     stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "cls_loss_backward");
}

int aarmvs_depth_metrics(const float* depth_est, const float* depth_gt, const float* mask, int B,
                         int HW, const float* thresholds, int n_thresholds, double* out,
                         void* scratch, hipStream_t stream) {
  if (!depth_est || !depth_gt || !mask || !out || !scratch || (n_thresholds > 0 && !thresholds))
    return fail(AARMVS_ERR_INVALID, "depth_metrics: null pointer argument");
  if (int rc = cls_check("depth_metrics", B, HW)) return rc;
  if (n_thresholds < 0 || n_thresholds > AARMVS_MAX_THRESHOLDS)
    return fail(AARMVS_ERR_INVALID, "depth_metrics: at most 8 thresholds");
  hipError_t e = launch_depth_metrics(depth_est, depth_gt, mask, B, HW, thresholds, n_thresholds, out,
                                      scratch, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "depth_metrics");
}

// ---- point-cloud evaluation (cloud.hip) ----
static bool cloud_count_ok(long long n) { return n >= 0 && n < (1LL << 31); }
static bool cloud_cell_ok(double cell) { return std::isfinite(cell) && cell > 0.0; }

int aarmvs_cloud_keys(const float* xyz, long long n, const double* origin, double cell, long long* keys_out,
                      hipStream_t stream) {
  if (!cloud_count_ok(n)) return fail(AARMVS_ERR_INVALID, "cloud_keys: need 0 <= n < 2^31");
  if (!origin || (n > 0 && (!xyz || !keys_out)))
    return fail(AARMVS_ERR_INVALID, "cloud_keys: null pointer argument");
  if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
    return fail(AARMVS_ERR_INVALID, "cloud_keys: origin must be finite");
  if (!cloud_cell_ok(cell)) return fail(AARMVS_ERR_INVALID, "cloud_keys: cell must be finite and > 0");
  if (n > 0 && ranges_overlap(keys_out, 8 * (size_t)n, xyz, 12 * (size_t)n))
    return fail(AARMVS_ERR_INVALID, "cloud_keys: keys_out must not alias xyz");
  hipError_t e = launch_cloud_keys(xyz, n, origin, cell, keys_out, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "cloud_keys");
}

int aarmvs_cloud_nn(const aarmvs_cloud_nn_args* a, hipStream_t stream) {
  if (!a) return fail(AARMVS_ERR_INVALID, "cloud_nn: null args");
  if (!cloud_count_ok(a->nq) || !cloud_count_ok(a->m))
    return fail(AARMVS_ERR_INVALID, "cloud_nn: need 0 <= nq, m < 2^31");
  if ((a->nq > 0 && (!a->query || !a->dist_out)) || (a->m > 0 && (!a->target || !a->target_keys)))
    return fail(AARMVS_ERR_INVALID, "cloud_nn: null pointer argument");
  if (!std::isfinite(a->origin[0]) || !std::isfinite(a->origin[1]) || !std::isfinite(a->origin[2]))
    return fail(AARMVS_ERR_INVALID, "cloud_nn: origin must be finite");
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
  hipError_t e = launch_cloud_nn(a, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "cloud_nn");
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
  hipError_t e = launch_cloud_stats(dist, n, thresholds, n_thresholds, out, scratch, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "cloud_stats");
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
  hipError_t e = launch_cloud_voxel_centroids(sorted_xyz, sorted_keys, n, out_xyz, capacity, count, workspace,
                                              stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "cloud_voxel_centroids");
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
  if (!std::isfinite(a->origin[0]) || !std::isfinite(a->origin[1]) || !std::isfinite(a->origin[2]))
    return fail(AARMVS_ERR_INVALID, "cloud_thin: origin must be finite");
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
  hipError_t e = launch_cloud_thin(a, rounds, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "cloud_thin");
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
  hipError_t e = launch_cloud_regions(xyz, n, mask, dims, bb, res, patch, plane, flags_out, stream);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, "cloud_regions");
}

}  // extern "C"
