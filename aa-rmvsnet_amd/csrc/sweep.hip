// The sweep's entry points, host code only: the forward sweep (aarmvs_sweep*) on the stream
// schedule of sweep_schedule.h, its backward (aarmvs_sweep_backward) and the single-plane pieces
// aarmvs_cost_slice and aarmvs_unet_step.  The kernels are in the cost, regulariser and head units.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "aarmvs_internal.h"

using namespace aarmvs;

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

static int check_precision(const char* who, int p) {
  if (p == AARMVS_PREC_SPLIT || p == AARMVS_PREC_FP16) return AARMVS_OK;
  return fail(AARMVS_ERR_INVALID, std::string(who) + ": unknown precision " + std::to_string(p) +
                                      " (AARMVS_PREC_SPLIT = 0, AARMVS_PREC_FP16 = 1)");
}

static bool src_complete(const float* const* src, int nsrc) {
  for (int v = 0; v < nsrc; ++v)
    if (!src[v]) return false;
  return true;
}

static bool record_complete(const aarmvs_train_record* r) {
  return r->x && r->state && r->z && r->u && r->stats && r->t1 && r->ostats;
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

// The c8 feature copies of the cost stage.  Each copy also folds 8 max|feature|^2 into ws.xbound
// (cell 0's fp16 range guard), which the caller has zeroed: with a memset of its own or, at the
// start of a sweep, with the statistics clear (ws.stats_bytes spans xbound).
static int feature_copies(const char* who, const float* ref, const float* const* src, int nsrc, int B, int HW,
                          const Workspace& ws, hipStream_t stream) {
  hipError_t e = launch_to_c8(ref, ws.feat8[0], B, HW, stream, ws.xbound);
  for (int v = 0; v < nsrc && e == hipSuccess; ++v)
    e = launch_to_c8(src[v], ws.feat8[1 + v], B, HW, stream, ws.xbound);
  return e == hipSuccess ? AARMVS_OK : hip_fail(e, (std::string(who) + ": c8 copy").c_str());
}

static CostArgs cost_args(const float* ref, const float* const* src, int nsrc, const float* rel,
                          const float* depth_values, const void* packed_params) {
  CostArgs ca{};
  ca.ref = ref;
  for (int v = 0; v < nsrc; ++v) ca.src[v] = src[v];
  ca.rel = rel;
  ca.depth_values = depth_values;
  ca.params = static_cast<const float*>(packed_params);
  return ca;
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
  int rc = check_precision("sweep", precision);
  if (rc) return rc;
  if (precision == AARMVS_PREC_FP16 && a->record)
    return fail(AARMVS_ERR_INVALID,
                "sweep: AARMVS_PREC_FP16 is an inference mode; a training record needs AARMVS_PREC_SPLIT "
                "(the backward differentiates the split cells)");
  if ((rc = check_geom(a->B, a->H, a->W, a->nsrc))) return rc;
  if (a->C != kC) return fail(AARMVS_ERR_INVALID, "sweep: feature channels C must be 32");
  if (a->D < 1 || a->d_begin < 0 || a->d_end > a->D || a->d_begin >= a->d_end)
    return fail(AARMVS_ERR_INVALID, "sweep: need 0 <= d_begin < d_end <= D");
  if (!a->ref_fea || !a->rel_proj || !a->depth_values || !a->packed_params || !a->workspace)
    return fail(AARMVS_ERR_INVALID, "sweep: null pointer argument");
  if (!src_complete(a->src_fea, a->nsrc)) return fail(AARMVS_ERR_INVALID, "sweep: null src_fea pointer");
  const aarmvs_train_record* rec = a->record;
  if (rec && !record_complete(rec)) return fail(AARMVS_ERR_INVALID, "sweep: training record with a null buffer");
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
  hipError_t e;
  const CostArgs ca = cost_args(a->ref_fea, a->src_fea, a->nsrc, a->rel_proj, a->depth_values, a->packed_params);
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
    // c8 copies of the features for the cost stage (the stats init above has cleared ws.xbound)
    if ((rc = feature_copies("sweep", a->ref_fea, a->src_fea, a->nsrc, a->B, a->H * a->W, ws, stream))) return rc;
  } else if (rec) {
    // A recorded call that starts inside the sweep (a later d_range piece, or the recompute of a
    // checkpointed segment) stands on its own: of what the d_begin == 0 branch prepares, record
    // mode reads the state from the record (slab d_begin - record_d0, the caller's), takes its
    // statistics in the record (zeroed below and per group in launch_omega_group) and needs the
    // WTA images only for depth_out / conf_out; what is left are the c8 feature copies and the
    // guard bound, re-made here as aarmvs_sweep_backward does (the workspace may have served
    // another sweep since; the same values when it has not)
    if ((e = hipMemsetAsync(ws.xbound, 0, sizeof(unsigned), stream)) != hipSuccess)
      return hip_fail(e, "sweep: bound init");
    if ((rc = feature_copies("sweep", a->ref_fea, a->src_fea, a->nsrc, a->B, a->H * a->W, ws, stream))) return rc;
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
  if (!record_complete(rec)) return fail(AARMVS_ERR_INVALID, "sweep_backward: training record with a null buffer");
  if (!src_complete(a->src_fea, a->nsrc))
    return fail(AARMVS_ERR_INVALID, "sweep_backward: null src_fea pointer");
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
  if ((e = hipMemsetAsync(ws.xbound, 0, sizeof(unsigned), stream)) != hipSuccess)
    return hip_fail(e, "sweep_backward: bound init");
  if ((rc = feature_copies("sweep_backward", a->ref_fea, a->src_fea, a->nsrc, a->B, a->H * a->W, ws, stream)))
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
  if (!src_complete(src_fea, nsrc)) return fail(AARMVS_ERR_INVALID, "cost_slice: null src_fea pointer");
  // one plane of the sweep's cost-slice pipeline (D = 1, depth_values = depth_d [B,1])
  SweepGeom g{B, H, W, nsrc, 1, cu_count()};
  Workspace ws = carve_workspace(workspace, B, H, W, nsrc);
  const CostArgs ca = cost_args(ref_fea, src_fea, nsrc, rel_proj, depth_d, packed_params);
  hipError_t e;
  const int HW = H * W;
  if ((e = hipMemsetAsync(ws.xbound, 0, sizeof(unsigned), stream)) != hipSuccess)
    return hip_fail(e, "cost_slice: bound init");
  if ((rc = feature_copies("cost_slice", ref_fea, src_fea, nsrc, B, HW, ws, stream))) return rc;
  if ((e = launch_omega_group(ca, g, ws, 0, 1, stream)) != hipSuccess)
    return hip_fail(e, "cost_slice: omega stage");
  if ((e = launch_cost_x_group(ca, g, ws, 0, 1, ws.x, omega_out, 0, stream)) != hipSuccess)
    return hip_fail(e, "cost_slice: cost slice");
  return launched(launch_layout(ws.x, slice_out, B, kC, HW, false, stream), "cost_slice: slice copy");
}

int aarmvs_unet_step(const float* x, int B, int H, int W, int nsrc, int step,
                     const void* packed_params, void* workspace, float* cost_out,
                     hipStream_t stream) {
  return aarmvs_unet_step_p(x, B, H, W, nsrc, step, packed_params, workspace, cost_out, AARMVS_PREC_SPLIT, stream);
}

int aarmvs_unet_step_p(const float* x, int B, int H, int W, int nsrc, int step,
                       const void* packed_params, void* workspace, float* cost_out, int precision,
                       hipStream_t stream) {
  int rc = check_precision("unet_step", precision);
  if (rc) return rc;
  if ((rc = check_geom(B, H, W, nsrc))) return rc;
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
  return launched(launch_head_wta(params, g, io, ws, nullptr, 0, cost_out, false, stream), "unet_step: head");
}

}  // extern "C"
