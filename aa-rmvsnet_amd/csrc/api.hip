// The core of libaarmvs's C ABI (include/aarmvs.h), host code only: the thread's error string,
// the kernel timer, the workspace carve with the geometry check and the size queries, and the
// library's stream pool.  Every other entry point sits in its op's unit, below the launcher it
// calls (the sweep's in sweep.hip, the parameter packing in pack_params.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "aarmvs_internal.h"

namespace aarmvs {

// the one error string of the thread, whichever unit's entry point failed (aarmvs_last_error)
static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int hip_fail(hipError_t e, const char* where) {
  return fail(AARMVS_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
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

int check_geom(int B, int H, int W, int nsrc) {
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

hipError_t library_stream(int dev, int i, hipStream_t& out) {
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
  return launched(e, "aux_stream");
}

float* aarmvs_state_ptr(void* workspace, int B, int H, int W, int nsrc, int planes,
                        int cell, int which) {
  if (!workspace || cell < 0 || cell > 4 || planes < 0 || check_geom(B, H, W, nsrc) != AARMVS_OK)
    return nullptr;
  Workspace ws = carve_workspace(workspace, B, H, W, nsrc);
  return which == 0 ? ws.h[cell][h_slot(cell, planes)] : ws.c[cell];
}

}  // extern "C"
