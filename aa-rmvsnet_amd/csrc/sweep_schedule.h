// The sweep's stream schedule, as a host-side description without HIP types: which stream
// each stage runs on (plan_sweep) and the order of its launches, event records and event waits
// (walk_sweep).  aarmvs_sweep (sweep.hip) executes it on HIP; tests/sweep_schedule_check.cpp walks
// it with a recording sink and checks, on the CPU, that every pair of conflicting buffer
// accesses is ordered for every unit -> stream map.
//
// Cost stage.  Planes are processed in groups of up to kPlaneGroup (AARMVS_NPL=n for A/B runs).
// The cost slices do not depend on the recurrence, so a group's whole cost-slice stage (omega
// conv, statistics, cost_x: one launch each over the group's planes) runs ahead of its
// regulariser steps.  Two-stream schedule (the caller gives an aux stream): the cost stage runs
// on the aux stream, group i's beside group i-1's regulariser steps on the caller's stream; per
// group parity two events: ev_cost[p] "group's slices ready" (aux -> caller's) and ev_used[p]
// "group's slices consumed" (caller's -> aux, before group i+2 reuses the slots).
//
// Multi-stream regulariser.  The U-Net step is five units run in order (U0 cell 0, U1 cell 1,
// U2 cell 2, U3 deconv_0 + cell 3, U4 deconv_1 + cell 4 and the head); a unit of plane d needs
// the earlier units of plane d and its own state only, so the units of neighbouring planes can
// run at once on different streams (stream 0 the caller's, the others library-owned).  Per unit
// and plane an event (a ring of kRegEvRing per unit):
//   data: a unit waits for the previous unit of its plane when that ran on another stream;
//   slots: unit k < 4 overwrites h_k's slot of plane d - kHRing[k]; it waits for that plane's
//   last reader of h_k when that ran on another stream (h0: U4, h1: U3, h2: U3, h3: U4; h4 is
//   read by U4's own head).  The other readers of the slot finished before the last one (the
//   data waits chain a plane's units).  c_k, u0, u1, the deconv partials and the WTA images
//   each have one unit as their only reader and writer.
//   A call that continues a sweep (d_begin > 0) skips the waits on planes before d_begin: the
//   earlier call joined them onto the caller's stream, and this call's forks start after it.
// Bit-identical to one stream (the same kernels on the same inputs).
// How many streams: a process gets GPU_MAX_HW_QUEUES = 4 hardware queues here, and streams
// beyond that share them (a stream waiting on an event then blocks the other's work), so a
// sweep uses at most four: with an aux stream (the caller asks for concurrency), the cost stage
// on it and the units on three (the caller's + two library streams: cells 0-1 | cell 2,
// deconv_0, cell 3 | deconv_1, cell 4, head).  Small frames (B*H*W <= kSmallFramePx) instead
// put the cost stage on the caller's stream beside cells 0-1 and the other units on the aux
// stream and two library streams (cell 2 | deconv_0, cell 3 | deconv_1, cell 4, head), still
// four streams (the library's are shared with the backward, library_stream): their kernels are a few
// microseconds of one or two tiles per block, so the chain's latency, not the cost stage, is
// what overlapping hides (config 1: 0.279 -> 0.334 G hyp/s, profiles/r06o_small_frames.txt).
// A training forward (with its record) takes 3 unit streams by default too (config-4 training
// step 251.4 -> 243.3 ms, profiles/r06m_train_streams.txt).  Under stream capture (a caller
// recording the sweep into a graph) everything stays on the caller's stream: the captured graph
// is the one-stream order, bit-identical to every schedule.
// Overrides (A/B runs): AARMVS_REG_STREAMS=1..5 the unit stream count (AARMVS_REG_STREAMS_REC for
// a training forward), AARMVS_REG_MAP five digits unit -> stream (unit 0 on stream 0),
// AARMVS_SMALL_PX the small-frame threshold.
// Library streams 1..3 are unit (or backward) streams and library stream 4 is the one
// aarmvs_aux_stream returns.  Five unit streams without the small-frame swap therefore put unit
// stream 4 on library stream 4: when the caller's aux stream came from aarmvs_aux_stream, unit 4
// and the cost stage share one queue (in order, so still correct; an A/B override only).
#pragma once

namespace aarmvs {

constexpr int kPlaneGroup = 16;
// the regulariser step's five units, run in that order: cell 0 | cell 1 | cell 2 |
// deconv_0 + cell 3 | deconv_1 + cell 4 (and the head)
constexpr int kUnetUnits = 5;
// hidden-state ring lengths: h_k of plane e is overwritten by plane e + kHRing[k], so the
// multi-stream regulariser's unit writing h_k may run up to kHRing[k] - 1 planes ahead of the
// last unit that reads it (h0: cell 4, four units on; h1: cell 3; h2: deconv_0; h3: deconv_1)
constexpr int kHRingMax = 6;
constexpr int kHRing[5] = {6, 4, 3, 3, 2};
inline int h_slot(int k, int e) { return e % kHRing[k]; }

constexpr int kRegMaxStreams = 5, kRegEvRing = 8;
static_assert(kRegEvRing > kHRingMax, "a unit's event is re-recorded only after its waiters are enqueued");
constexpr int kHLastReader[4] = {4, 3, 3, 4};
constexpr long kSmallFramePx = 65536;
// the stream of each unit for n streams (row n - 1)
constexpr int kUnitStream[kRegMaxStreams][kUnetUnits] = {
    {0, 0, 0, 0, 0}, {0, 0, 0, 1, 1}, {0, 0, 1, 1, 2}, {0, 0, 1, 2, 3}, {0, 1, 2, 3, 4}};

// Stream slots: 0 .. nreg - 1 the units' streams (0 the caller's), kAuxSlot the cost stage's own.
enum SweepStream : int { kNoStream, kCaller, kCallerAux, kLib1, kLib2, kLib3, kLib4 };
constexpr int kAuxSlot = kRegMaxStreams, kSweepSlots = kRegMaxStreams + 1;

// Events, as indices into one set: per group parity ev_cost and ev_used, the aux slot's
// fork/join event, per unit a ring over planes, per unit slot a fork/join event.
constexpr int kEvCost = 0, kEvUsed = 2, kEvAuxJoin = 4, kEvPart = 5,
              kEvRegJoin = kEvPart + kUnetUnits * kRegEvRing, kSweepEvents = kEvRegJoin + kRegMaxStreams;
inline int ev_part(int u, int d) { return kEvPart + u * kRegEvRing + d % kRegEvRing; }

struct SweepPlan {
  int nreg;                        // unit streams in use
  int unit_stream[kUnetUnits];     // slot of each unit
  int cost_slot;                   // kAuxSlot (the two-stream cost stage), or 0
  bool aux_to_units;               // small frames: the caller's aux stream is unit slot 1
  int G;                           // planes per group
  SweepStream slot[kSweepSlots];   // which stream each slot is
  bool events() const { return cost_slot != 0 || nreg > 1; }
};

// An environment override, already parsed (AARMVS_REG_MAP as its text), or absent.
struct SweepOpt {
  bool set = false;
  long value = 0;
};
struct SweepOverrides {
  SweepOpt reg_streams, reg_streams_rec, small_px, npl;
  const char* reg_map = nullptr;
};

// aux: the caller gave an aux stream other than its stream; px = B*H*W.
inline SweepPlan plan_sweep(bool aux, bool capturing, bool recording, long px, const SweepOverrides& o) {
  auto clamp = [](long v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : (int)v; };
  SweepPlan p{};
  if (capturing) aux = false;
  const bool small = aux && px <= (o.small_px.set ? o.small_px.value : kSmallFramePx);
  int n = 1;
  if (!capturing) {
    const SweepOpt& s = recording ? o.reg_streams_rec : o.reg_streams;
    n = clamp(s.set ? s.value : (!aux ? 1 : small ? 4 : 3), 1, kRegMaxStreams);
  }
  for (int u = 0; u < kUnetUnits; ++u) p.unit_stream[u] = kUnitStream[n - 1][u];
  p.nreg = n;
  // a map: five digits below kRegMaxStreams, the first 0; anything else is ignored
  if (const char* m = n > 1 ? o.reg_map : nullptr) {
    int len = 0, top = 0;
    bool ok = m[0] == '0';
    for (; m[len]; ++len) {
      ok = ok && len < kUnetUnits && m[len] >= '0' && m[len] < '0' + kRegMaxStreams;
      if (ok && m[len] - '0' > top) top = m[len] - '0';
    }
    if (ok && len == kUnetUnits) {
      for (int u = 0; u < kUnetUnits; ++u) p.unit_stream[u] = m[u] - '0';
      p.nreg = top + 1;
    }
  }
  // small frames: the cost stage on the caller's stream, the aux stream one of the units' streams
  p.aux_to_units = small && p.nreg > 3;
  p.cost_slot = aux && !p.aux_to_units ? kAuxSlot : 0;
  p.G = clamp(o.npl.set ? o.npl.value : kPlaneGroup, 1, kPlaneGroup);
  p.slot[0] = kCaller;
  for (int i = 1, li = 0; i < p.nreg; ++i)
    p.slot[i] = i == 1 && p.aux_to_units ? kCallerAux : SweepStream(kLib1 + li++);
  if (p.cost_slot) p.slot[kAuxSlot] = kCallerAux;
  return p;
}

struct SweepGroup {
  int gi, g0, n;   // index within the call (its parity picks the slice slots), first plane, planes
};

// Emits one call's forks, stages and joins to the sink, in enqueue order.  Sink methods return
// 0 or an error code, which ends the walk and is returned:
//   fork(slot, ev)  record ev on slot 0, make `slot` wait for it
//   join(slot, ev)  record ev on `slot`, make slot 0 wait for it
//   wait(slot, ev), record(slot, ev)
//   cost_group(slot, grp)   the cost stage of the group's planes
//   slice_copy(grp, d)      the cost slice of plane d copied out, on slot 0
//   step(grp, d)            all five units and the head of plane d, on slot 0
//   unit(slot, u, grp, d), head(slot, d)
// Once the forks have succeeded, every return (errors included) is preceded by the joins:
// everything the call enqueued on another slot is ordered on slot 0.
template <class Sink>
int walk_sweep_groups(const SweepPlan& p, int d_begin, int d_end, int slice_plane, Sink& s) {
  const bool aux = p.cost_slot != 0;
  int rc;
  SweepGroup grp{0, d_begin, 0};
  for (; grp.g0 < d_end; grp.g0 += p.G, ++grp.gi) {
    grp.n = d_end - grp.g0 < p.G ? d_end - grp.g0 : p.G;
    const int par = grp.gi & 1;
    // cost stage: its slots were last read by group gi - 2's regulariser steps
    if (aux && grp.gi >= 2 && (rc = s.wait(kAuxSlot, kEvUsed + par))) return rc;
    if ((rc = s.cost_group(p.cost_slot, grp))) return rc;
    if (aux && ((rc = s.record(kAuxSlot, kEvCost + par)) || (rc = s.wait(0, kEvCost + par)))) return rc;
    // regulariser steps and WTA of the group's planes
    for (int d = grp.g0; d < grp.g0 + grp.n; ++d) {
      if (d == slice_plane && (rc = s.slice_copy(grp, d))) return rc;
      if (p.nreg == 1) {
        if ((rc = s.step(grp, d))) return rc;
        continue;
      }
      for (int u = 0; u < kUnetUnits; ++u) {
        const int su = p.unit_stream[u];
        // wait for unit q of plane e on another stream (planes before this call: joined)
        auto wait_unit = [&](int q, int e) {
          return e < d_begin || p.unit_stream[q] == su ? 0 : s.wait(su, ev_part(q, e));
        };
        if (u > 0 && (rc = wait_unit(u - 1, d))) return rc;
        // the hidden-state slot this unit overwrites, last read kHRing planes back
        if (u < 4 && (rc = wait_unit(kHLastReader[u], d - kHRing[u]))) return rc;
        if ((rc = s.unit(su, u, grp, d))) return rc;
        if (u == kUnetUnits - 1 && (rc = s.head(su, d))) return rc;
        if ((rc = s.record(su, ev_part(u, d)))) return rc;
      }
    }
    if (aux && (rc = s.record(0, kEvUsed + par))) return rc;
  }
  return 0;
}

template <class Sink>
int walk_sweep(const SweepPlan& p, int d_begin, int d_end, int slice_plane, Sink& s) {
  const bool aux = p.cost_slot != 0;
  int rc = aux ? s.fork(kAuxSlot, kEvAuxJoin) : 0;
  for (int i = 1; i < p.nreg && !rc; ++i) rc = s.fork(i, kEvRegJoin + i);
  if (rc) return rc;   // nothing is enqueued on the other slots yet
  rc = walk_sweep_groups(p, d_begin, d_end, slice_plane, s);
  // every slot is joined, whatever failed before; the first error is the call's
  auto first = [&](int r) { rc = rc ? rc : r; };
  if (aux) first(s.join(kAuxSlot, kEvAuxJoin));
  for (int i = 1; i < p.nreg; ++i) first(s.join(i, kEvRegJoin + i));
  return rc;
}

}  // namespace aarmvs
