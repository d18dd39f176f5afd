// CPU check of the sweep's stream schedule (aa-rmvsnet_amd/csrc/sweep_schedule.h): walks the
// plan with a recording sink, simulates happens-before between streams and events, and checks
// that every pair of conflicting buffer accesses is ordered, that every event wait resolves to
// the record it means, and that every call ends with all its work ordered on the caller's
// stream.  It proves ordering of the buffers modelled here (the reads and writes of
// launch_unet_step, launch_head_wta and the cost stage); it says nothing about the runtime
// (tests/test_gpu_streams.py runs the same scenarios on the device).
//
// Two sweeps in flight (check_two_sweeps): two callers with their own buffers and their own
// streams issue their calls alternately from one host thread, so that the library's streams and
// ONE event array serve both.  Each sweep must still pass every check above.
//
// Happens-before: each stream keeps the set of ops known complete before its next launch; a
// launch inherits the set and joins it; a record snapshots the set; a wait merges the snapshot
// the event held when the wait was enqueued.
#include <bitset>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../aa-rmvsnet_amd/csrc/sweep_schedule.h"

using namespace aarmvs;

namespace {

constexpr int kD = 40, kMaxOps = 1024, kPhys = 7, kK = 48;   // kK > kD + 1: per-plane buffer indices
constexpr int kCallerB = 6;   // the second caller's stream (two sweeps in flight)
using Set = std::bitset<kMaxOps>;

// buffer ids: per-cell [5][kK], per-plane [kK], then the single buffers
enum : int {
  B_H = 0, B_C = 5 * kK, B_X = 10 * kK, B_T1 = 11 * kK, B_OSTATS = 12 * kK, B_U = 13 * kK /* [2] */,
  B_STATS = 15 * kK /* [2] */, B_COST = 17 * kK, B_FEAT8 = 18 * kK, B_PART /* [2] */, B_WTA = B_PART + 2,
  kBufs
};

enum EvKind : int { E_NONE, E_FORK, E_COST, E_USED, E_PART };
struct Tag {
  EvKind kind = E_NONE;
  int a = 0, b = 0;   // E_COST / E_USED: group index; E_PART: unit, plane
  bool operator==(const Tag& o) const { return kind == o.kind && a == o.a && b == o.b; }
};

int g_failed = 0;
#define CHECK(c, ...)                                         \
  do {                                                        \
    if (!(c)) {                                               \
      if (++g_failed <= 20) {                                 \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
        std::printf(__VA_ARGS__);                             \
        std::printf("\n");                                    \
      }                                                       \
    }                                                         \
  } while (0)

// One sweep (one or more calls) on simulated streams; or two sweeps, each with its caller's
// stream and (unless told to share) its buffer set, on the same library streams and events.
struct Sim {
  bool record_model;   // a training record: per-plane slabs for x, h, c, u, stats, t1, omega stats
  bool alias;          // the caller's aux stream is library stream 4
  const SweepPlan* plan = nullptr;
  int d_begin = 0, call = -1, gi = 0, last_u = 0, last_d = 0;
  int nops = 0, op_phys[kMaxOps] = {}, op_owner[kMaxOps] = {};
  int caller = 0, owner = 0;   // the current call's caller stream and sweep
  Set done[kPhys];
  struct Ev { Set snap; Tag tag; int call = -1; } ev[kSweepEvents];
  struct BufState { int writer = -1; Set readers; } sets[2][kBufs];
  BufState* bufs = sets[0];
  struct Pending { int ev; Tag tag; } pend[8];
  int npend = 0;
  int hazards = 0, event_errors = 0;

  Sim(bool rec, bool al) : record_model(rec), alias(al) {}

  // the calls that follow belong to `sweep`, issued on caller stream `stream`
  void use(int sweep, int stream, bool rec, bool shared_bufs) {
    owner = sweep;
    caller = stream;
    record_model = rec;
    bufs = sets[shared_bufs ? 0 : sweep];
  }

  int phys(int slot) {
    switch (plan->slot[slot]) {
      case kCaller: return caller;
      case kCallerAux: return alias ? 5 : 1;
      case kLib1: return 2;
      case kLib2: return 3;
      case kLib3: return 4;
      case kLib4: return 5;
      default: ++event_errors; return 0;   // a slot without a stream
    }
  }
  // --- buffers
  int h(int k, int e) const { return B_H + k * kK + (record_model ? e : e % kHRing[k]); }
  int c(int k, int e) const { return B_C + k * kK + (record_model ? e : 0); }
  int plane(int base, int d) const { return base + (record_model ? d : 0); }
  int x(const SweepGroup& g, int d) const { return B_X + (record_model ? d : g.gi & 1); }

  int launch(int p) {
    const int op = nops++;
    if (op >= kMaxOps) { std::printf("too many ops\n"); std::exit(2); }
    op_phys[op] = p;
    op_owner[op] = owner;
    return op;
  }
  void finish(int op) { done[op_phys[op]].set(op); }
  void acc(int op, int id, bool write) {
    BufState& b = bufs[id];
    const Set& before = done[op_phys[op]];
    if (b.writer >= 0 && b.writer != op && !before[b.writer]) ++hazards;
    if (write) {
      Set r = b.readers;
      r.reset(op);
      if ((r & ~before).any()) ++hazards;
      b.writer = op;
      b.readers.reset();
    } else {
      b.readers.set(op);
    }
  }
  void rd(int op, int id) { acc(op, id, false); }
  void wr(int op, int id) { acc(op, id, true); }

  // the reads and writes of unit u of plane d (launch_unet_step) and of the head
  void unit_acc(int op, int u, const SweepGroup& g, int d) {
    static const int reads[5][2] = {{-1, -1}, {0, -1}, {1, -1}, {2, 1}, {3, 0}};   // h_k[d + 1]
    if (u == 0) rd(op, x(g, d));
    for (int k : reads[u])
      if (k >= 0) rd(op, h(k, d + 1));
    rd(op, h(u, d));
    rd(op, c(u, d));
    if (u >= 3) {
      wr(op, plane(B_U + (u - 3) * kK, d));
      wr(op, B_PART + (u - 3));
      wr(op, plane(B_STATS + (u - 3) * kK, d));
    }
    wr(op, h(u, d + 1));
    wr(op, c(u, d + 1));
  }
  void head_acc(int op, int d) {
    rd(op, h(4, d + 1));
    wr(op, B_WTA);
    wr(op, B_COST + d);
  }

  // --- one call: the d_begin == 0 initialisation, the walk, finalize; then the join check
  template <class Sink>
  int run_call(const SweepPlan& p, int d0, int d1, Sink& s) {
    plan = &p;
    d_begin = d0;
    ++call;
    npend = 0;
    if (d0 == 0) {   // the memsets and c8 copies, on the caller's stream
      const int op = launch(caller);
      for (int k = 0; k < 5; ++k) {
        for (int e = 0; e < (record_model ? 1 : kHRing[k]); ++e) wr(op, h(k, e));
        wr(op, c(k, 0));
      }
      wr(op, B_WTA);
      wr(op, B_OSTATS);
      wr(op, B_FEAT8);
      finish(op);
    }
    const int rc = walk_sweep(p, d0, d1, d1 - 1, s);
    if (!rc) {
      CHECK(npend == 0, "waits left without their launch");
      const int op = launch(caller);   // finalize
      rd(op, B_WTA);
      finish(op);
    }
    return rc;
  }
  // the current sweep's ops not ordered on its caller's stream, those of stream `except` aside
  int count_unjoined(int except = -1) const {
    int n = 0;
    for (int op = 0; op < nops; ++op) n += op_owner[op] == owner && !done[caller][op] && op_phys[op] != except;
    return n;
  }

  // --- the sink
  void do_record(int p, int i, Tag t) {
    ev[i].snap = done[p];
    ev[i].tag = t;
    ev[i].call = call;
  }
  void do_wait(int p, int i) {
    if (ev[i].call != call) ++event_errors;   // not recorded in this call
    done[p] |= ev[i].snap;
  }
  int fork(int slot, int i) {
    do_record(caller, i, {E_FORK, 0, 0});
    do_wait(phys(slot), i);
    return 0;
  }
  int join(int slot, int i) {
    do_record(phys(slot), i, {E_FORK, 0, 0});
    do_wait(caller, i);
    return 0;
  }
  int record(int slot, int i) {
    const int par = gi & 1;
    Tag t;
    if (i == kEvCost + par) t = {E_COST, gi, 0};
    else if (i == kEvUsed + par) t = {E_USED, gi, 0};
    else if (i >= kEvPart && i < kEvRegJoin) t = {E_PART, last_u, last_d};
    else ++event_errors;
    do_record(phys(slot), i, t);
    return 0;
  }
  int wait(int slot, int i) {
    if (i >= kEvCost && i < kEvCost + 2) {
      if (!(ev[i].tag == Tag{E_COST, gi, 0})) ++event_errors;
    } else if (npend < 8) {
      pend[npend++] = {i, ev[i].tag};   // judged when the launch it guards arrives
    } else {
      ++event_errors;
    }
    do_wait(phys(slot), i);
    return 0;
  }
  int cost_group(int slot, const SweepGroup& g) {
    for (int j = 0; j < npend; ++j)
      if (!(pend[j].tag == Tag{E_USED, g.gi - 2, 0}) || pend[j].ev != kEvUsed + (g.gi & 1)) ++event_errors;
    npend = 0;
    gi = g.gi;
    const int op = launch(phys(slot));
    rd(op, B_FEAT8);
    for (int d = g.g0; d < g.g0 + g.n; ++d) {
      wr(op, x(g, d));
      wr(op, plane(B_T1, d));
      wr(op, plane(B_OSTATS, d));
    }
    finish(op);
    return 0;
  }
  int slice_copy(const SweepGroup& g, int d) {
    const int op = launch(caller);
    rd(op, x(g, d));
    finish(op);
    return 0;
  }
  int step(const SweepGroup& g, int d) {
    if (npend) ++event_errors;
    const int op = launch(caller);
    for (int u = 0; u < kUnetUnits; ++u) unit_acc(op, u, g, d);
    head_acc(op, d);
    finish(op);
    return 0;
  }
  int unit(int slot, int u, const SweepGroup& g, int d) {
    for (int j = 0; j < npend; ++j) {   // each wait resolves to the record of the unit and plane it means
      const int q = (pend[j].ev - kEvPart) / kRegEvRing;
      const int e = q == u - 1 ? d : (u < 4 && q == kHLastReader[u]) ? d - kHRing[u] : -1;
      if (pend[j].ev < kEvPart || pend[j].ev >= kEvRegJoin || e < d_begin || !(pend[j].tag == Tag{E_PART, q, e}))
        ++event_errors;
    }
    npend = 0;
    const int op = launch(phys(slot));
    unit_acc(op, u, g, d);
    finish(op);
    last_u = u;
    last_d = d;
    return 0;
  }
  int head(int slot, int d) {
    const int op = launch(phys(slot));
    head_acc(op, d);
    finish(op);
    return 0;
  }
};

// Wait classes a Filter can drop (the production header has no such hook), and an error it can
// inject at the n-th sink call.
enum WaitClass : int { W_NONE = -1, W_DATA = 0 /* + u, 1..4 */, W_SLOT = 5 /* + u, 0..3 */, W_COST = 9, W_USED = 10, kWaitClasses };
struct Filter {
  Sim& sim;
  int drop = W_NONE, fail_at = -1;
  int calls = 0, failed_join_slot = -1;
  struct Held { int slot, ev; } held[8] = {};
  int nheld = 0;

  bool fails() { return calls++ == fail_at; }
  int fork(int slot, int i) { return fails() ? 7 : sim.fork(slot, i); }
  int join(int slot, int i) {
    if (fails()) {
      failed_join_slot = slot;
      return 7;
    }
    return sim.join(slot, i);
  }
  int record(int slot, int i) { return fails() ? 7 : sim.record(slot, i); }
  int wait(int slot, int i) {
    if (fails()) return 7;
    if (i >= kEvPart && i < kEvRegJoin && drop != W_NONE) {   // its class shows at the unit it guards
      held[nheld++] = {slot, i};
      return 0;
    }
    if ((drop == W_COST && i < kEvCost + 2) || (drop == W_USED && i >= kEvUsed && i < kEvUsed + 2)) return 0;
    return sim.wait(slot, i);
  }
  int cost_group(int slot, const SweepGroup& g) { return fails() ? 7 : sim.cost_group(slot, g); }
  int slice_copy(const SweepGroup& g, int d) { return fails() ? 7 : sim.slice_copy(g, d); }
  int step(const SweepGroup& g, int d) { return fails() ? 7 : sim.step(g, d); }
  int unit(int slot, int u, const SweepGroup& g, int d) {
    if (fails()) return 7;
    for (int j = 0; j < nheld; ++j) {
      const int q = (held[j].ev - kEvPart) / kRegEvRing;
      const int cls = q == u - 1 ? W_DATA + u : W_SLOT + u;
      if (cls != drop) sim.wait(held[j].slot, held[j].ev);
    }
    nheld = 0;
    return sim.unit(slot, u, g, d);
  }
  int head(int slot, int d) { return fails() ? 7 : sim.head(slot, d); }
};

const int kCuts[3][5] = {{0, kD, -1}, {0, 1, 16, kD, -1}, {0, 7, kD, -1}};

struct Case {
  bool aux, capturing, recording;
  long px;
  SweepOverrides o;
};
SweepPlan plan_of(const Case& c) { return plan_sweep(c.aux, c.capturing, c.recording, c.px, c.o); }
SweepOpt opt(long v) { return SweepOpt{true, v}; }

bool uses(const SweepPlan& p, SweepStream id) {
  for (SweepStream s : p.slot)
    if (s == id) return true;
  return false;
}

// One sweep cut into calls; returns the hazards found (0 when dropping nothing is the claim).
int run_sweep(const Case& c, const int* cut, bool alias, int drop, long* runs) {
  auto sim = std::make_unique<Sim>(c.recording, alias);
  int bad = 0;
  for (int i = 0; cut[i + 1] >= 0; ++i) {
    const SweepPlan p = plan_of(c);   // per call, as aarmvs_sweep does
    Filter f{*sim, drop};
    Sim& direct = *sim;
    const int rc = drop == W_NONE ? sim->run_call(p, cut[i], cut[i + 1], direct) : sim->run_call(p, cut[i], cut[i + 1], f);
    bad += rc != 0;
    bad += sim->count_unjoined();
  }
  ++*runs;
  return sim->hazards + (drop == W_NONE ? sim->event_errors + bad : 0);
}

// Two sweeps in flight from one host thread: sweep 0 on caller stream 0, sweep 1 on kCallerB, the
// pieces of the two issued alternately.  Both callers' aux stream is the library's (alias), the
// library streams and the event array are the same for both; each has its buffer set unless
// shared_bufs (the use the contract forbids: it must show as a hazard).
int run_two_sweeps(const Case& ca, const Case& cb, const int* cut, bool shared_bufs, long* runs) {
  auto sim = std::make_unique<Sim>(false, true);
  int bad = 0;
  for (int i = 0; cut[i + 1] >= 0; ++i)
    for (int w = 0; w < 2; ++w) {
      const Case& c = w ? cb : ca;
      sim->use(w, w ? kCallerB : 0, c.recording, shared_bufs);
      const SweepPlan p = plan_of(c);   // per call, as aarmvs_sweep does
      bad += sim->run_call(p, cut[i], cut[i + 1], *sim) != 0;
      bad += sim->count_unjoined();     // the call ends joined on its own caller's stream
    }
  ++*runs;
  return sim->hazards + sim->event_errors + bad;
}

// every default plan beside itself and beside the plain small-frame sweep (an eval sweep next to
// a training forward among them), every cut
void check_two_sweeps(long* runs) {
  const long npl[4] = {0, 1, 3, 16};
  const Case partner{true, false, false, 160L * 128, {}};
  for (int bits = 0; bits < 16; ++bits)
    for (int streams = 0; streams <= 5; ++streams)
      for (long n : npl) {
        Case c{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) ? 160L * 128 : 1600L * 1184, {}};
        if (streams) c.o.reg_streams = c.o.reg_streams_rec = opt(streams);
        if (n) c.o.npl = opt(n);
        for (const auto& cut : kCuts)
          for (int other = 0; other < 2; ++other) {
            const int bad = run_two_sweeps(c, other ? partner : c, cut, false, runs);
            CHECK(bad == 0, "two sweeps: %d unordered accesses / event errors / unjoined ops (bits %d streams %d npl %ld, "
                  "cut %d.., partner %d)", bad, bits, streams, n, cut[1], other);
          }
      }
  // not vacuous: the same two sweeps on ONE buffer set race, under both default plans
  for (long px : {160L * 128, 1600L * 1184}) {
    const Case c{true, false, false, px, {}};
    long unused = 0;
    const int n = run_two_sweeps(c, c, kCuts[1], true, &unused);
    std::printf("two sweeps on one buffer set (%ld px): %d hazards\n", px, n);
    CHECK(n > 0, "two sweeps sharing their buffers go unnoticed (%ld px)", px);
  }
}

// every cut, with the caller's aux stream distinct from library stream 4 and equal to it
// (one run where the plan does not use both)
int check_case(const Case& c, const char* what, long* runs) {
  const SweepPlan p = plan_of(c);
  const bool both = uses(p, kCallerAux) && uses(p, kLib4);
  int bad = 0;
  for (const auto& cut : kCuts)
    for (int alias = 0; alias <= (both ? 1 : 0); ++alias) {
      const int n = run_sweep(c, cut, alias != 0, W_NONE, runs);
      CHECK(n == 0, "%s: %d unordered accesses / event errors (map %d%d%d%d%d nreg %d cost slot %d, cut %d.., alias %d)",
            what, n, p.unit_stream[0], p.unit_stream[1], p.unit_stream[2], p.unit_stream[3], p.unit_stream[4],
            p.nreg, p.cost_slot, cut[1], alias);
      bad += n;
    }
  return bad;
}

void map_text(int m, char (&s)[6]) {   // m in 0 .. 624: units 1..4 in base 5, unit 0 on stream 0
  s[0] = '0';
  for (int u = 4; u >= 1; --u, m /= 5) s[u] = char('0' + m % 5);
  s[5] = 0;
}

void check_all_maps(long* runs) {
  // the map applies once a call has more than one unit stream: with an aux stream (large frame:
  // cost stage on it; small frame: the aux stream handed to the units), or forced by the override
  Case base[3] = {{true, false, false, 1600L * 1184, {}}, {true, false, false, 160L * 128, {}}, {false, false, false, 1600L * 1184, {}}};
  base[2].o.reg_streams = base[2].o.reg_streams_rec = opt(5);
  for (Case c : base)
    for (int rec = 0; rec < 2; ++rec)
      for (int m = 0; m < 625; ++m) {
        char text[6];
        map_text(m, text);
        c.recording = rec != 0;
        c.o.reg_map = text;
        const SweepPlan p = plan_of(c);
        bool same = true;
        for (int u = 0; u < kUnetUnits; ++u) same = same && p.unit_stream[u] == text[u] - '0';
        CHECK(same, "map %s not taken", text);
        check_case(c, "map", runs);
      }
}

void check_defaults(long* runs) {
  const long npl[4] = {0, 1, 3, 16};
  for (int bits = 0; bits < 16; ++bits)
    for (int streams = 0; streams <= 5; ++streams)
      for (long n : npl) {
        Case c{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) ? 160L * 128 : 1600L * 1184, {}};
        if (streams) c.o.reg_streams = c.o.reg_streams_rec = opt(streams);
        if (n) c.o.npl = opt(n);
        check_case(c, "default", runs);
      }
}

// input -> expected plan
void check_plans() {
  struct Row {
    const char* what;
    Case c;
    int nreg, us[kUnetUnits], cost_slot;
    bool aux_to_units;
    SweepStream slot[kSweepSlots];
  };
  const long big = 1600L * 1184, small = 160L * 128;
  SweepOverrides bad_len, bad_first, bad_digit, good, five, small_px, zero, huge;
  bad_len.reg_map = "0012";
  bad_first.reg_map = "10123";
  bad_digit.reg_map = "00125";
  good.reg_map = "01021";
  five.reg_streams = opt(5);
  small_px.small_px = opt(big);
  zero.reg_streams = opt(0);
  huge.reg_streams = opt(99);
  const Row rows[] = {
      {"capture: one stream, no aux", {true, true, false, small, five}, 1, {0, 0, 0, 0, 0}, 0, false, {kCaller}},
      {"no aux: one unit stream", {false, false, false, big, {}}, 1, {0, 0, 0, 0, 0}, 0, false, {kCaller}},
      {"aux, large: three unit streams, cost on aux", {true, false, false, big, {}}, 3, {0, 0, 1, 1, 2}, kAuxSlot, false,
       {kCaller, kLib1, kLib2, kNoStream, kNoStream, kCallerAux}},
      {"aux, large, recording", {true, false, true, big, {}}, 3, {0, 0, 1, 1, 2}, kAuxSlot, false,
       {kCaller, kLib1, kLib2, kNoStream, kNoStream, kCallerAux}},
      {"aux, small: four, aux is unit stream 1, cost on the caller's", {true, false, false, small, {}}, 4, {0, 0, 1, 2, 3}, 0,
       true, {kCaller, kCallerAux, kLib1, kLib2}},
      {"aux, exactly kSmallFramePx is small", {true, false, false, kSmallFramePx, {}}, 4, {0, 0, 1, 2, 3}, 0, true,
       {kCaller, kCallerAux, kLib1, kLib2}},
      {"aux, one pixel more is large", {true, false, false, kSmallFramePx + 1, {}}, 3, {0, 0, 1, 1, 2}, kAuxSlot, false,
       {kCaller, kLib1, kLib2, kNoStream, kNoStream, kCallerAux}},
      {"AARMVS_SMALL_PX moves the threshold", {true, false, false, big, small_px}, 4, {0, 0, 1, 2, 3}, 0, true,
       {kCaller, kCallerAux, kLib1, kLib2}},
      {"five streams, large: unit 4 on library stream 4", {true, false, false, big, five}, 5, {0, 1, 2, 3, 4}, kAuxSlot, false,
       {kCaller, kLib1, kLib2, kLib3, kLib4, kCallerAux}},
      {"five streams, small", {true, false, false, small, five}, 5, {0, 1, 2, 3, 4}, 0, true,
       {kCaller, kCallerAux, kLib1, kLib2, kLib3}},
      {"five streams, no aux", {false, false, false, big, five}, 5, {0, 1, 2, 3, 4}, 0, false,
       {kCaller, kLib1, kLib2, kLib3, kLib4}},
      {"the recording override is its own", {true, false, true, big, five}, 3, {0, 0, 1, 1, 2}, kAuxSlot, false,
       {kCaller, kLib1, kLib2, kNoStream, kNoStream, kCallerAux}},
      {"stream count clamped up", {true, false, false, big, zero}, 1, {0, 0, 0, 0, 0}, kAuxSlot, false,
       {kCaller, kNoStream, kNoStream, kNoStream, kNoStream, kCallerAux}},
      {"stream count clamped down", {false, false, false, big, huge}, 5, {0, 1, 2, 3, 4}, 0, false,
       {kCaller, kLib1, kLib2, kLib3, kLib4}},
      {"map of the wrong length ignored", {true, false, false, big, bad_len}, 3, {0, 0, 1, 1, 2}, kAuxSlot, false,
       {kCaller, kLib1, kLib2, kNoStream, kNoStream, kCallerAux}},
      {"map with unit 0 off stream 0 ignored", {true, false, false, big, bad_first}, 3, {0, 0, 1, 1, 2}, kAuxSlot, false,
       {kCaller, kLib1, kLib2, kNoStream, kNoStream, kCallerAux}},
      {"map with a digit >= 5 ignored", {true, false, false, big, bad_digit}, 3, {0, 0, 1, 1, 2}, kAuxSlot, false,
       {kCaller, kLib1, kLib2, kNoStream, kNoStream, kCallerAux}},
      {"a map sets the stream count", {true, false, false, big, good}, 3, {0, 1, 0, 2, 1}, kAuxSlot, false,
       {kCaller, kLib1, kLib2, kNoStream, kNoStream, kCallerAux}},
      {"a map needs more than one stream", {false, false, false, big, good}, 1, {0, 0, 0, 0, 0}, 0, false, {kCaller}},
      {"small, a map below four streams keeps the cost stage on aux", {true, false, false, small, good}, 3, {0, 1, 0, 2, 1},
       kAuxSlot, false, {kCaller, kLib1, kLib2, kNoStream, kNoStream, kCallerAux}},
  };
  for (const Row& r : rows) {
    const SweepPlan p = plan_of(r.c);
    bool ok = p.nreg == r.nreg && p.cost_slot == r.cost_slot && p.aux_to_units == r.aux_to_units && p.G == kPlaneGroup;
    for (int u = 0; u < kUnetUnits; ++u) ok = ok && p.unit_stream[u] == r.us[u];
    for (int i = 0; i < kSweepSlots; ++i) ok = ok && p.slot[i] == r.slot[i];
    CHECK(ok, "plan: %s", r.what);
  }
  SweepOverrides o;
  const long npl_in[5] = {-3, 0, 1, 3, 99}, npl_out[5] = {1, 1, 1, 3, kPlaneGroup};
  for (int i = 0; i < 5; ++i) {
    o.npl = opt(npl_in[i]);
    CHECK(plan_sweep(true, false, false, big, o).G == npl_out[i], "AARMVS_NPL=%ld", npl_in[i]);
  }
}

// an error at each sink call of one short walk: the call still ends joined
void check_join_on_error() {
  Case c{true, false, false, 1600L * 1184, {}};
  c.o.npl = opt(2);
  c.o.reg_map = "01234";
  const SweepPlan p = plan_of(c);
  int total = 0;
  {
    Sim sim(false, false);
    Filter f{sim};
    CHECK(sim.run_call(p, 0, 5, f) == 0 && sim.count_unjoined() == 0, "clean short walk");
    total = f.calls;
  }
  CHECK(total > 100, "short walk has %d sink calls", total);
  for (int alias = 0; alias < 2; ++alias)
    for (int k = 0; k < total; ++k) {
      auto sim = std::make_unique<Sim>(false, alias != 0);
      Filter f{*sim, W_NONE, k};
      const int rc = sim->run_call(p, 0, 5, f);
      CHECK(rc == 7, "error at call %d returned %d", k, rc);
      // a join that fails itself leaves that one stream's work behind, nothing else
      const int except = f.failed_join_slot >= 0 ? sim->phys(f.failed_join_slot) : -1;
      const int n = sim->count_unjoined(except);
      CHECK(n == 0, "error at call %d (alias %d): %d ops not ordered on the caller's stream", k, alias, n);
    }
}

// dropping all waits of one class must show as a hazard for at least one map
void check_not_vacuous() {
  Case c{true, false, false, 1600L * 1184, {}};
  for (int cls = 0; cls < kWaitClasses; ++cls) {
    if (cls == W_DATA) continue;   // unit 0 has no data wait
    int caught = 0;
    long runs = 0;
    for (int m = 0; m < 625; ++m) {
      char text[6];
      map_text(m, text);
      c.o.reg_map = text;
      caught += run_sweep(c, kCuts[0], false, cls, &runs) > 0;
    }
    std::printf("wait class %2d dropped: caught by %d of 625 maps\n", cls, caught);
    CHECK(caught > 0, "dropping wait class %d goes unnoticed", cls);
  }
}

}  // namespace

int main() {
  long runs = 0;
  check_plans();
  check_all_maps(&runs);
  check_defaults(&runs);
  check_two_sweeps(&runs);
  check_join_on_error();
  check_not_vacuous();
  std::printf("sweep_schedule_check: %ld sweeps simulated, %d failed checks\n", runs, g_failed);
  if (!g_failed) std::printf("sweep_schedule_check: ok\n");
  return g_failed ? 1 : 0;
}
