// Internal declarations shared by the HIP translation units of libaarmvs.
// Layouts of the packed parameter buffer and of the sweep workspace live here.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/aarmvs.h"
#include "sweep_schedule.h"

namespace aarmvs {

constexpr int kC = 32;          // feature channels (FeatNet output)
constexpr int kSlots = 32;      // fp64 atomic slots per GroupNorm statistic
constexpr float kGnEps = 1e-5f; // nn.GroupNorm default eps
// The sweep computes cost slices in groups of up to kPlaneGroup planes (sweep_schedule.h): one
// launch of each cost-slice kernel covers the group, so the neighbouring planes' bilinear
// footprints (and the reference tile) are fetched from HBM once and re-read from L2.

// ---------------------------------------------------------------------------
// Parameter tensors, in raw-blob order (aarmvs.h).
// ---------------------------------------------------------------------------
enum ParamId : int {
  P_OW0, P_OB0, P_OG0W, P_OG0B, P_OW1, P_OB1, P_OG1W, P_OG1B, P_OW2, P_OB2, P_OG2W, P_OG2B,
  P_OWO, P_OBO,
  P_C0W, P_C0B, P_C1W, P_C1B, P_C2W, P_C2B, P_C3W, P_C3B, P_C4W, P_C4B,
  P_D0W, P_D0B, P_D0GW, P_D0GB, P_D1W, P_D1B, P_D1GW, P_D1GB,
  P_HW, P_HB,
  P_COUNT
};

constexpr int kParamSize[P_COUNT] = {
    4 * 32 * 9, 4, 4, 4, 16, 4, 4, 4, 16, 4, 4, 4, 4, 1,
    64 * 48 * 9, 64, 64 * 32 * 9, 64, 64 * 32 * 9, 64, 64 * 48 * 9, 64, 32 * 40 * 9, 32,
    16 * 16 * 9, 16, 16, 16, 16 * 16 * 9, 16, 16, 16,
    8 * 9, 1};

// LSTM cell geometry (drmvsnet.py:241-244): input x-channels, hidden channels, scale.
constexpr int kCellCX[5] = {32, 16, 16, 32, 32};
constexpr int kCellHid[5] = {16, 16, 16, 16, 8};
constexpr int kCellScale[5] = {1, 2, 4, 2, 1};

// Split-fp16 MFMA operands of a cell's conv weights (see convlstm.hip): input channels
// padded to a multiple of 16 (one 16-channel chunk per k-group), A fragments ordered
// [chunk][tap][m-tile][lane][8 halves], hi then lo.
__host__ __device__ constexpr int cell_cin(int k) { return kCellCX[k] + kCellHid[k]; }
__host__ __device__ constexpr int cell_chunks(int k) { return (cell_cin(k) + 15) / 16; }
__host__ __device__ constexpr int cell_a_halves(int k) {   // per hi / lo
  return cell_chunks(k) * 9 * (kCellHid[k] / 8) * 64 * 8;
}
// BPTT input-gradient conv of cell k: K = 4 hid gate channels (16-channel chunks), M = cin
// rows in 32-row m-tiles; halves per m-tile (hi and lo)
__host__ __device__ constexpr int dg_chunks(int k) { return 4 * kCellHid[k] / 16; }
__host__ __device__ constexpr int dg_mtiles(int k) { return (cell_cin(k) + 31) / 32; }
__host__ __device__ constexpr int dg_mt_halves(int k) { return dg_chunks(k) * 9 * 2 * 64 * 8; }

struct ParamLayout {
  size_t raw_off[P_COUNT];
  size_t pk_off[P_COUNT];   // packed offsets (floats), 64-float aligned
  size_t h3_off[5];         // split-fp16 cell weights (hi then lo halves), in floats; taps with
                            // (tap + chunk) odd negated (the training cells' sign balance)
  size_t h3p_off[5];        // the same, every tap positive (the inference cells)
  size_t h3_scale_off;      // 5 floats: 1 / (power-of-two weight scale) per cell
  size_t ow0t_off;          // omega conv3x3 weights as [tap][ci][co] (1,152 floats)
  size_t owb_scale_off;     // 1 float: 1 / (power-of-two scale of the omega conv fragments)
  size_t owm_off;           // omega conv3x3 off-centre taps as split-fp16 v_mfma_f32_32x32x16_f16
                            // B fragments [chunk][2][64 lanes][8] (omega_mfma; same scale)
  size_t dct_off[2];        // deconv_0/1 weights as [ci][tap][co] (2,304 floats each)
  size_t dcm_off[2];        // deconv_0/1 as split-fp16 v_mfma_f32_32x32x16_f16 A fragments
                            // [6 tap pairs][hi, lo][64 lanes][8 halves], then 1 float: 2^-e
                            // (the fragments carry the power-of-two weight scale 2^e)
  size_t dg_off[5];         // BPTT: each cell's input-gradient conv (the forward conv
                            // transposed: taps flipped, in/out channels swapped) as split-fp16
                            // A fragments [m-tile][chunk][tap][hi, lo][64 lanes][8 halves]
  size_t dg_scale_off;      // 5 floats: 1 / (power-of-two scale) of those fragments
  size_t raw_total;
  size_t pk_total;
};
const ParamLayout& param_layout();

// ---------------------------------------------------------------------------
// Workspace layout.
// ---------------------------------------------------------------------------
struct Workspace {
  double* omega_stats;    // [kPlaneGroup][B][nsrc][3][kSlots][2] omega GN statistics per group plane
  double* omega_part;     // [kPlaneGroup][B][nsrc][omega_part_n][2] per-block GN partial sums
  int omega_part_n;       // partials per (plane, b, view): >= omega tiles, >= statistics blocks
  double* reg_stats;      // [B][2 deconvs][2 groups][kSlots][2] U-Net GN statistics
  double* reg_part;       // [B][deconv_1 blocks][4] deconv_1's per-block GN partials
  double* reg_part0;      // [B][deconv_0 blocks][4] deconv_0's (its own region: the two deconvs
                          // of neighbouring planes may run at once on the regulariser's streams)
  unsigned* xbound;       // float bits of an upper bound on |x| (cost slice) for this sweep:
                          // 8 max|feature|^2 (to_c8) or max|x| (unet_step); cell 0's fp16 range
  float* max_prob;        // [B,HW]
  float* exp_sum;         // [B,HW]
  float* depth;           // [B,HW]
  float* xg[2];           // per group parity: [kPlaneGroup][B][H][W][32] cost slices (NHWC)
  float* x;               // = xg[0]: the single-slice buffer of aarmvs_unet_step / cost_slice
  float* feat8[AARMVS_MAX_SRC + 1]; // [B][4][H][W][8] "c8" copies of ref (0) and source views
  float* t1;              // [kPlaneGroup][B][nsrc][HW][4] omega conv3x3 output per group plane
  float* u0;              // [B,16,H/2,W/2] deconv_0 output (pre-GN)
  float* u1;              // [B,16,H,W]     deconv_1 output (pre-GN)
  float* h[5][kHRingMax]; // hidden states: a ring of kHRing[k] slots (plane d reads slot d % r
                          // and writes slot (d + 1) % r)
  float* h_pool[2][kHRingMax]; // maxpool2x2 of h[0] / h[1]'s slots (a quarter their size): part of
                          // the slot -- same index, written by the same unit, waited on by the
                          // same event; past the zero-initialised state region (cells 1 and 2
                          // read only what cells 0 and 1 of the same plane wrote)
  float* c[5];            // cell states (updated in place)
  size_t bytes;
  size_t omega_stats_bytes;  // one plane
  size_t reg_stats_bytes;
  size_t stats_bytes;        // omega + reg statistics and xbound (contiguous, for the initial clear)
  size_t state_bytes;        // h[*][*], c[*] region (contiguous) for zero-init
  void* state_begin;
  size_t wta_bytes;          // max_prob/exp_sum/depth region
  size_t x_plane;            // floats per plane in xg
  size_t t1_plane;           // float4s per plane in t1
};
Workspace carve_workspace(void* base, int B, int H, int W, int nsrc);
// U-Net statistic (deconv j, group g) of batch element b within reg_stats
__host__ __device__ inline size_t reg_stat_index(int b, int j, int g) {
  return ((size_t)(b * 2 + j) * 2 + g) * kSlots * 2;
}

// ---------------------------------------------------------------------------
// Kernel launchers (defined in the .hip units).
// ---------------------------------------------------------------------------
struct SweepGeom {
  int B, H, W, nsrc, D;
  int cu_count;
};

hipError_t launch_pack_params(const float* raw, float* packed, hipStream_t s);

struct CostArgs {
  const float* ref;
  const float* src[AARMVS_MAX_SRC];
  const float* rel;       // [nsrc][B][12]
  const float* depth_values;  // [B,D]
  const float* params;    // packed
};
// The cost-slice stage (cost_fwd.hip) for the planes d0 .. d0 + n - 1 (n <= kPlaneGroup):
// omega_group clears the group's statistics, then writes t1 and the three GroupNorm
// statistics of every plane (omega conv + omega_stats<1> + <2>); cost_x_group then writes
// each plane's cost slice to x0 + k ws.x_plane (and, for plane omega_k, the omega weights
// to omega_out).  Both use the t1 / statistics slots of the workspace: one group at a time.
// launch_layout: NCHW <-> NHWC copy of a [B][C][HW] / [B][HW][C] fp32 tensor (API edges only);
// xmax (optional, to_nhwc only): atomic max of |in| as float bits
hipError_t launch_layout(const float* in, float* out, int B, int C, int HW, bool to_nhwc,
                         hipStream_t s, unsigned* xmax = nullptr);
// xbound (optional): atomic max of 8 max|src|^2 as float bits, an upper bound on the cost
// slice's |x| (|warp - ref| <= 2 max|feature|, (1 + w) <= 2)
hipError_t launch_to_c8(const float* src, float* dst, int B, int HW, hipStream_t s,
                        unsigned* xbound = nullptr);
hipError_t launch_omega_group(const CostArgs& a, const SweepGeom& g, const Workspace& ws, int d0,
                              int n, hipStream_t s,
                              bool balanced = false);
hipError_t launch_cost_x_group(const CostArgs& a, const SweepGeom& g, const Workspace& ws, int d0,
                               int n, float* x0, float* omega_out, int omega_k, hipStream_t s);

// Where one regulariser step reads and writes its tensors (all NHWC): the eval sweep's
// workspace ping-pong (c updated in place) or a training record's per-plane slabs
// (unet_io_ws / unet_io_record).
struct UnetIO {
  const float* h_prev[5];
  float* h_new[5];
  float* h_pool[2];     // maxpool2x2(h_new[0 / 1]) [B][Hk/2][Wk/2][16], written by cells 0 and 1 for
                        // cells 1 and 2, or null (training record: the consumers pool h_new)
  const float* c_prev[5];
  float* c_new[5];
  float* z[5];          // gate pre-activations [B][Hk][Wk][4 hid], or null (eval)
  float* u0;            // deconv_0 output [B][H/2][W/2][16] (pre-GN)
  float* u1;            // deconv_1 output [B][H][W][16]
  double* reg_stats;    // the two deconvs' GroupNorm statistics (reg_stat_index layout)
  bool clear_stats;     // the head kernel zeroes reg_stats after use (eval: one shared set)
};

// Training record (aarmvs_train_record, include/aarmvs.h): per-plane slabs, in floats
// (stats in doubles).  A state slab holds h then c of every cell; slab 0 is the zero initial
// state (drmvsnet.py:133-134), slab d + 1 the state after plane d.
struct TrainLayout {
  size_t x_plane;
  size_t state_slab, h_off[5], c_off[5];
  size_t z_slab, z_off[5];
  size_t u_slab, u0_off, u1_off;
  size_t stats_slab;   // doubles
  size_t cell_px[5];   // B * pixels of cell k
};
TrainLayout train_layout(int B, int H, int W);
UnetIO unet_io_ws(const Workspace& ws, int d);   // plane d (absolute index in the sweep)
UnetIO unet_io_record(const TrainLayout& T, const aarmvs_train_record& r, int d);

// stages: the step's five units (bit u = unit u, run in that order: cell 0 | cell 1 | cell 2 |
// deconv_0 + cell 3 | deconv_1 + cell 4); a unit of plane d reads only the earlier units'
// outputs of plane d and its own state, so the units of neighbouring planes may run at once on
// different streams (the sweep's multi-stream regulariser).  precision: aarmvs_precision -- the
// split cells and deconvs (three fp16 products per fp32 product) or, for inference steps only
// (no io.z), their 1-product fp16 variants
constexpr int kUnetAll = (1 << kUnetUnits) - 1;
hipError_t launch_unet_step(const float* x, const float* params, const SweepGeom& g,
                            const Workspace& ws, const UnetIO& io, hipStream_t s,
                            int stages = kUnetAll, int precision = AARMVS_PREC_SPLIT);
hipError_t launch_head_wta(const float* params, const SweepGeom& g, const UnetIO& io,
                           const Workspace& ws, const float* depth_values, int d,
                           float* cost_out, bool wta, hipStream_t s, void* refine_state = nullptr,
                           void* posterior_state = nullptr);
// ^ refine_state: the sub-plane refinement's per-pixel state (16 B per pixel) or null; non-null
// launches the refining instantiation of the head kernel.  posterior_state: likewise the
// depth-posterior statistics' state (16 B per pixel), independent of the former
hipError_t launch_finalize(const SweepGeom& g, const Workspace& ws, float* depth_out,
                           float* conf_out, hipStream_t s);
// the sweep's opt-in outputs after n planes, from the WTA images and the per-pixel state: the
// sub-plane refinement, and the depth-posterior statistics (mean, std, entropy, runner-up)
hipError_t launch_refine_finalize(const float* max_prob, const float* exp_sum, const float* depth,
                                  const void* state, const float* depth_values, int B, int D, int n,
                                  int HW, float* depth_refined, float* conf_window, int* index,
                                  hipStream_t s);
hipError_t launch_posterior_finalize(const float* exp_sum, const void* state, int B, int HW,
                                     float* mean, float* sd, float* entropy, float* runner_up,
                                     hipStream_t s);

// ---------------------------------------------------------------------------
// The ABI boundary's shared pieces.  The thread's error string lives in api.hip alone
// (aarmvs_last_error reads it): every unit's entry points report through these.
// ---------------------------------------------------------------------------
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* where);
int check_geom(int B, int H, int W, int nsrc);
// the tail of an entry point that makes one launch
inline int launched(hipError_t e, const char* who) { return e == hipSuccess ? AARMVS_OK : hip_fail(e, who); }
// [p, p + n) and [q, q + m) share a byte
inline bool ranges_overlap(const void* p, size_t n, const void* q, size_t m) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + m && b < a + n;
}

int cu_count();

// Per-device host state (func attributes, aux streams and events) is kept in arrays indexed by
// the current device, so that one process driving several devices (nn.DataParallel) gets each
// device its own.
constexpr int kMaxDevices = 64;
inline hipError_t current_device(int& dev) {
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess && (dev < 0 || dev >= kMaxDevices)) e = hipErrorInvalidDevice;
  return e;
}
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per device for a kernel
inline hipError_t ensure_dyn_lds(const void* fn, int bytes, bool (&done)[kMaxDevices]) {
  int dev = 0;
  hipError_t e = current_device(dev);
  if (e != hipSuccess || done[dev]) return e;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done[dev] = true;
  return e;
}
// The library's own streams (i = 1 .. kLibStreams), created on first use per device and shared
// by every call of the process, from any host thread (sweeps: the regulariser's unit streams;
// backward: the plane pipeline's and the group stage's).  A process gets GPU_MAX_HW_QUEUES = 4
// hardware queues here and every stream it creates holds one, so streams beyond four share a
// queue, where one stream's event wait stalls the other's work: the library keeps the process's
// total (the caller's stream and aux stream included) at four.  Calls on different host threads
// that share a stream are only ordered, never mixed: each call's events are its thread's own.
constexpr int kLibStreams = 4;   // 1-3: unit / backward streams; 4: aarmvs_aux_stream
hipError_t library_stream(int dev, int i, hipStream_t& out);
// Joins an auxiliary stream back into the caller's stream when it goes out of scope: on every
// return after a fork (errors included), nothing the call enqueued on the aux stream is left
// unordered with the caller's stream, whose buffers the caller may free on an error.
struct StreamJoin {
  hipStream_t main, aux;
  hipEvent_t ev;
  hipError_t join() {   // order the aux stream's work so far on main (once)
    hipError_t e = hipSuccess;
    if (aux && aux != main && ev) {
      e = hipEventRecord(ev, aux);
      if (e == hipSuccess) e = hipStreamWaitEvent(main, ev, 0);
    }
    aux = nullptr;
    return e;
  }
  ~StreamJoin() { (void)join(); }
};

// Backward of the regulariser (bptt.hip) over every plane of a training record: the
// parameter gradients of the cells / deconvs / head into the fp64 accumulators of its scratch
// (written to grad_params as float at the end, the cost-slice part included if group_done
// adds to them), and per group of planes dL/dx handed to group_done (planes g0 .. g0 + n - 1,
// gx [n][B][H][W][32]) and copied to grad_x if set.
struct BpttRun {
  int B, H, W, D;
  // The planes of this call, [d_begin, d_end): multiples of kPlaneGroup (d_end may be D), so
  // that the groups are those of the whole backward.  One backward is a chain of calls, last
  // range first: the one with d_end == D zeroes the state gradients and the accumulators in
  // `scratch`, the others continue from what the call before left there, and the one with
  // d_begin == 0 writes grad_params.  `rec` is indexed by the absolute plane.
  int d_begin, d_end;
  const float* packed;
  const aarmvs_train_record* rec;
  const float* grad_cost;      // [B][D][H][W]
  const unsigned* xbound;      // float bits of a bound on |x| (the forward's fp16 guard bound)
  void* scratch;               // bptt_scratch_bytes
  float* grad_x;               // optional [D][B][H][W][32]
  float* grad_params;          // optional [raw count]
  hipError_t (*group_done)(void* ctx, int g0, int n, const float* gx, hipStream_t s);
  void* ctx;
};
size_t bptt_scratch_bytes(int B, int H, int W);
hipError_t bptt_regulariser(const BpttRun& r, hipStream_t s);
// the fp64 parameter-gradient accumulators inside a bptt scratch buffer
double* bptt_gacc(void* scratch, int B, int H, int W);

// Backward of the cost-slice stage (cost_bwd.hip): per group of planes, from dL/dx to the
// omega.* parameter gradients (into gacc) and dL/d features (accumulated, written out by
// cost_bwd_end).
struct CostBwdCtx {
  const aarmvs_backward_args* a;
  Workspace ws;
  void* scratch;      // cost_bwd_scratch_bytes
  double* gacc;       // the regulariser's fp64 accumulators (raw layout)
};
size_t cost_bwd_scratch_bytes(int B, int H, int W, int nsrc);
hipError_t cost_bwd_begin(CostBwdCtx& c, hipStream_t s);
hipError_t cost_bwd_group(void* ctx, int g0, int n, const float* gx, hipStream_t s);
hipError_t cost_bwd_end(CostBwdCtx& c, hipStream_t s);

// ---------------------------------------------------------------------------
// Opt-in per-kernel timing (aarmvs_profile_*): hipEvents recorded on the launch
// stream around each kernel.  Off by default; costs nothing when off.
// ---------------------------------------------------------------------------
enum KernelId : int {
  K_COST_X, K_OMEGA_CONV, K_FUSION, K_OMEGA1, K_OMEGA2,
  K_CELL0, K_CELL1, K_CELL2, K_CELL3, K_CELL4,
  K_DECONV0, K_DECONV1, K_HEAD_WTA, K_FINALIZE, K_SOFTMAX, K_WARP, K_TO_C8, K_STAT_REDUCE,
  K_GN_REDUCE, K_EVIDENTIAL,
  // the training backward (bptt.hip, the cbw_* kernels of cost_bwd.hip)
  K_GATE_BWD0, K_GATE_BWD1, K_GATE_BWD2, K_GATE_BWD3, K_GATE_BWD4,
  K_DGRAD0, K_DGRAD1, K_DGRAD2, K_DGRAD3, K_DGRAD4,
  K_WGRAD0, K_WGRAD1, K_WGRAD2, K_WGRAD3, K_WGRAD4,
  K_GNB_PARTIAL, K_DECONV_BWD, K_BWD_SMALL, K_CBW_CHAIN, K_CBW_FEAT, K_CBW_SMALL,
  K_DECONV_WGRAD, K_HEAD_WGRAD, K_DEFORM,
  K_PYR_DOWN, K_FUSION_POINTS,
  K_CLS_LOSS_FWD, K_CLS_LOSS_REDUCE, K_CLS_LOSS_BWD, K_DEPTH_METRICS,
  // the fp16 mode's 1-product cells and deconvs (AARMVS_PREC_FP16), in the order of K_CELL0 ..
  K_CELL0_FP16, K_CELL1_FP16, K_CELL2_FP16, K_CELL3_FP16, K_CELL4_FP16,
  K_DECONV0_FP16, K_DECONV1_FP16,
  K_REFINE,   // the sub-plane refinement's finalize and its from-the-volume kernel; the
              // depth-posterior statistics' two are counted here too (the list of names is fixed)
  K_COUNT
};
extern bool g_prof_on;
void prof_mark(hipStream_t s, int id, bool begin);
struct ProfScope {
  hipStream_t s;
  int id;
  ProfScope(hipStream_t s_, int id_) : s(s_), id(id_) {
    if (g_prof_on) prof_mark(s, id, true);
  }
  ~ProfScope() {
    if (g_prof_on) prof_mark(s, id, false);
  }
};

}  // namespace aarmvs
