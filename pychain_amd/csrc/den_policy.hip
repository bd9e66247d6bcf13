// den_policy.hip - what a denominator call runs and in which order: the recursion family of a call (den_decide_family), the
// DenArgs of the query entry points, time segments, rows exp'd ahead, and the schedules of the recursion and occupancy
// launches (run_den_launches).  No allocation, no host synchronisation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>

#include "../../include/pychain_hip.h"
#include "common.h"
#include "den_kernels.h"
#include "den_policy.h"

namespace pychain_hip {

int device_cu_count() {
  static std::mutex lock;
  static std::map<int, int> cus;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  std::lock_guard<std::mutex> guard(lock);
  auto it = cus.find(dev);
  if (it != cus.end()) return it->second;
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  return cus[dev] = n;
}

// One set per (device, caller's stream): two calls in flight on two streams of one device must not share
// the side streams' events (a second hipEventRecord would move the event the first call still waits for),
// and calls on ONE stream are ordered, so they may.  Entries live for the life of the process.
SideStream* side_streams_for(hipStream_t caller) {
  static std::map<std::pair<int, hipStream_t>, SideStream> table;
  static std::mutex create_lock;              // first use may come from several host threads
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> guard(create_lock);
  SideStream& s = table[std::make_pair(dev, caller)];
  if (!s.ready) {
    if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
    // stream2: den_exp_rows_kernel, whose rows the recursions wait for (dispatched first: highest priority), then the gate(s)
    // and the occupancy launches that overlap the recursions
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
    if (hipStreamCreateWithPriority(&s.stream2, hipStreamNonBlocking, greatest) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&s.fork, hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&s.join, hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&s.join2, hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) return nullptr;
    for (int i = 0; i < kMaxSegments; i++)
      if (hipEventCreateWithFlags(&s.seg[i], hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) return nullptr;
    s.ready = true;
  }
  return &s;
}

// ---- which recursion family a call runs ---------------------------------------------------------------------------------------
namespace {
// Two sequences per recursion workgroup (den_pair.inc.h) pay once the 2B one-sequence workgroups would fill the
// chip: the recursions then run on half of it and the occupancy launches and the numerator on the other half.
// Option den_pair: "1" wherever the shape allows (the tests), "0" never.
bool den_call_is_pair(const DenArgs& a, int hint, bool small) {
  if (!den_pair_eligible(a, hint)) return false;
  if (a.knobs.den_pair >= 0) return a.knobs.den_pair != 0;
  // small graphs run in four-wave workgroups, several to a CU: nothing to gain from pairing sequences
  if (a.knobs.den_lazy && small) return false;
  // measured on the C3 graph (round 5, 256 CUs).  Fused step: B = 96 one-sequence workgroups 4.40 ms, pairs 4.58; B = 104:
  // 5.36 / 4.58; B = 128: 6.60 / 5.24 - below about 100 sequences the one-sequence workgroups leave enough of the chip to the
  // occupancy launches and the numerator, and their chain is shorter.  The denominator ALONE has the chip to itself: one-
  // sequence workgroups while they all fit (B = 104: 3.77 against 4.63 with pairs, 112: 3.95 / 4.62, 128: 4.36 / 4.80)
  if (a.fused) return 64 * a.B >= 25 * device_cu_count();
  return 2 * a.B > device_cu_count();
}
}  // namespace

void den_decide_family(DenArgs& a, int hint) {
  a.pair = a.lazy = a.shape = a.sg = 0;
  if (hint == PYCHAIN_HIP_HINT_GENERAL) return;          // den_general.hip: rows in den_recursion_kernel's normalised form
  // the nnet-output rows of the lazy recursions come in by LDS-direct loads (default wherever a lazy shape fits: on the
  // 16-wave map of C3 it is 2 % faster than rows through registers and bit-identical, and it is what makes rows of
  // 4096 < D <= 9216 pdfs - C4 - fit a 128-VGPR wave at all); option den_dma = "0": rows through registers, i.e. the
  // 16-wave map for D <= 4096 and den_recursion_kernel beyond
  const bool small = a.knobs.den_dma != 0 && den_small_eligible(a, hint);
  const bool dma = a.knobs.den_dma != 0 && den_dma_eligible(a, hint);
  a.pair = den_call_is_pair(a, hint, small) ? 1 : 0;
  a.lazy = (a.knobs.den_lazy && !a.pair && (den_lazy_eligible(a, hint) || small || dma)) ? 1 : 0;
  if (a.lazy) a.shape = small ? kShapeSmall : (dma ? kShapeDma : kShapeRegs);
  a.sg = (a.lazy && a.shape == kShapeDma && den_sg_eligible(a, hint)) ? 1 : 0;   // (a "pdf by state" plan in the one-gather form)
}

void den_shape_args(DenArgs& a, int64_t plan_stride, int H, int D, int B, int T) {
  memset(&a, 0, sizeof(a));
  a.plan_stride = plan_stride;
  a.B = B; a.T = T; a.D = D; a.H = H; a.Hp = roundup64(H);
  a.frames_per_block = 32;      // measured at C3: 16 and 64 are both 1-3 % slower
  a.knobs = call_knobs();
  a.check_all = a.knobs.verbose >= 1 ? 1 : 0;
}

DenArgs den_query_args(int64_t plan_stride, int hint, int H, int D, int B, int T, bool fused, bool input_is_exp) {
  DenArgs a;
  den_shape_args(a, plan_stride, H, D, B, T);
  a.fused = fused ? 1 : 0;
  a.input_is_exp = input_is_exp ? 1 : 0;
  a.coef = 1e-5f;               // (the usual leaky-HMM coefficient: option den_q asks for one in [1e-8, 1])
  den_decide_family(a, hint);
  return a;
}

namespace {
// Number of time segments the denominator is cut into so that the occupancy pass of the frames
// whose alpha'/beta rows already exist runs on idle CUs WHILE the recursions continue
// (2B persistent workgroups leave the other CUs free).  1 = no overlap.
int den_segments(const DenArgs& a) {
  const int T = a.T;
  if (a.knobs.den_segments >= 1 && a.knobs.den_segments <= kMaxSegments) return a.knobs.den_segments;
  // What limits the overlap is CU time: after T/2 the occupancy pass has the ~128 idle CUs only (less the
  // numerator's), on which its ~1 ms of whole-chip work takes longer than the rest of the recursion, so
  // the last launch (the frames that only become computable at the very end) is exposed.  Each further
  // segment halves that launch but costs a launch (gate + kernel, ~0.05 ms of side-stream time).
  // Measured at C3 (T=1500), whole step, gated schedule with compact grids:
  //   3 -> 3.85 ms, 4 -> 3.74, 5 -> 3.81, 6 -> 3.90   (C4, T=2000: 3 -> 6.86, 4 -> 6.84, 5 -> 7.03)
  // (history: with one recursion launch per segment and full occupancy grids it was 3 -> 4.43, 4 -> 4.52)
  // shorter batches (B=64, same graph; ms per step for 1 / 2 / 3 / 4 segments): T=896: 2.79 / 2.71 / 2.42 / 2.37,
  // T=640: 2.01 / 1.93 / 1.72 / 1.72, T=384: 1.21 / 1.22 / 1.07 / 1.11
  if (T >= 768) return 4;
  if (T >= 256) return 3;
  // small graphs in four-wave workgroups leave most of the chip idle and their frames are short: the occupancy pass
  // overlaps from 64 frames on (C2, T = 150)
  if (a.lazy && a.shape == kShapeSmall && T >= 64) return 2;
  return 1;
}
}  // namespace

// Time segments (DenArgs::tseg): how many a call's (sequence, direction) recursions are cut into.  With few
// sequences the chain of T dependent frames IS the step and most CUs idle; S segments started `burn` frames outside
// themselves run T / S + burn frames each on 2 B S workgroups.  The price: the burn-in frames (CU-time) and the occupancy launch no
// longer overlapping the recursions (a frame's rows come from four workgroups, not two).  Chosen where the estimate says it
// pays by more than 5 %: per frame ~1.94 us (2.2 us for rows beyond 4096 pdfs), occupancy ~3.5 ps per frame and pdf of whole-chip
// time; the grid must leave every workgroup a CU (a fused call: half of the chip stays with the numerator).  The fused loss at
// B = 64 is never cut (CU-time-bound: DESIGN.md §4); the denominator alone at B = 64 runs two segments, C4 (B = 32) four.
int den_time_segments(const DenArgs& a, bool fused) {
  const int want = a.knobs.den_tseg;
  // (not a function of the verbose level: a debug run computes what production computes - ADVICE r5; the per-frame check of
  // verbose >= 1 reads the totals and occupancy sums a cut call stores like an uncut one)
  if (want == 0 || want == 1 || !a.lazy || a.shape != kShapeDma) return 1;
  const int burn = a.knobs.den_tburn;
  if (burn < 1) return 1;
  // (a fused call: a quarter of the chip stays with the numerator - measured on 256 CUs, the C3 graph: B = 24 in 4 segments
  // (192 workgroups) 1.58 ms against 2.25 in 2; B = 40 / 48 in 2 (160 / 192): 2.53 / 2.67 against 3.02 uncut; B = 32 in 4 (256): 2.59
  // against 2.41 in 2; B = 56 in 2 (224): as uncut)
  const int cus = fused ? device_cu_count() * 3 / 4 : device_cu_count();
  int best = 1;
  const double f = a.D > 4096 ? 2.2e-6 : 1.94e-6, occ = 3.5e-12 * (double)a.D * (double)a.B * (double)a.T;
  // (not cut: the chain, 5 % of head and tail, and the part of the streamed occupancy launch that is left when the recursions
  // end - about a third of it with sequences of one length; cut: the occupancy launch follows the recursions, + three launches)
  double best_t = 0.95 * (1.05 * (double)a.T * f + (fused ? 0.1 : 0.35) * occ);
  for (int S = 2; S <= kMaxTimeSegs; S *= 2) {
    // (a forced count only has to fit the chip: the segments wait for nobody)
    if (2 * a.B * S > (want == S ? device_cu_count() : cus) || a.T < 2 * burn) continue;
    if (want == S) return S;
    const double t = ((double)a.T / S + burn) * f + occ + 6e-5;
    if (want < 0 && t < best_t) { best = S; best_t = t; }
  }
  return best;
}

// Would a call of the denominator alone, given a workspace with the [B,T,D] buffer, exp its rows ahead of the recursions (§3.9)?
// The recursion workgroups spin on rows that launch writes and each takes a whole CU, so the
// launch must find CUs of its own whatever the order of dispatch: at least a quarter of the chip stays free of recursion
// workgroups, else the recursions exp their rows themselves (2B >= the CU count with pairing off could hang).
bool den_would_exp_rows_ahead(const DenArgs& a) {
  // (not where the call is cut into time segments: the rows are written from the sequence ends inwards, a segment starts inside;
  // not for the one-gather form of a "pdf by state" plan: its beta recursion reads its rows a frame ahead of the others)
  // (round 6: NOT for the 16-wave maps any more - since the rows' clamp / exp sits late in the arc phase and the frame lost a dozen
  // instructions, the recursions with their own rows are the faster ones in the only calls that still took them, the uncut ones of
  // 65 .. 96 sequences: C3 graph, denominator alone, B = 80: 3.35 -> 3.23 ms, B = 96: 4.0 -> 3.6 ms; C4's graph and rows, B = 80,
  // T <= 1000: 4.25 -> 3.25 ms (profiles/r06_rows_ahead.txt); four-wave workgroups keep them (C2: 0.208 against 0.214 ms); option
  // den_dma = 3: wherever the shape allows)
  const bool pays = a.shape == kShapeSmall || a.knobs.den_dma == 3;
  return a.lazy && !a.sg && (a.shape == kShapeDma || a.shape == kShapeSmall) && a.knobs.den_dma != 2 && pays && !a.input_is_exp &&
         a.D % 4 == 0 && a.D <= 4 * 5 * 512 && a.T >= 64 && 4 * den_recursion_blocks(a) <= 3 * device_cu_count() &&
         den_time_segments(a, false) == 1;
}

// 2-byte network outputs (DenArgs::x_half) are read as they are - and the gradient written in the same type - by the lazy
// recursions with LDS-direct rows, the pair recursion and both occupancy kernels in their float4-chunk forms; rows of a
// multiple of 8 pdfs (a lane's 16 raw bytes are 8 elements: all inside the row or all past it).  Every other kernel family
// (general plans, the two-barrier recursion, rows through registers, per-sequence plans of the gated schedule included)
// reads fp32: the caller up-casts (pychain_amd/native.py does).
bool den_call_half_native(const DenArgs& a0, int hint) {
  if (hint == PYCHAIN_HIP_HINT_GENERAL || a0.D % 8 != 0) return false;
  DenArgs a = a0;
  den_decide_family(a, hint);
  const bool rec_ok = a.pair || (a.lazy && (a.shape == kShapeDma || a.shape == kShapeSmall));
  return rec_ok && den_occupancy_half_ok(a, (a.D + 63) / 64, hint);
}

// ---- the schedules of one call's launches -------------------------------------------------------------------------------------
namespace {
// option debug_corrupt_row: one stored alpha row *= scale, between the recursion and the occupancy launches
__global__ void scale_row_kernel(float* row, int n, float scale) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) row[i] *= scale;
}
hipError_t launch_corrupt_row(const DenArgs& a, hipStream_t st) {
  float* row = a.alpha_store + ((size_t)a.knobs.corrupt_b * a.T + a.knobs.corrupt_t) * a.Hp;
  hipLaunchKernelGGL(scale_row_kernel, dim3(1), dim3(256), 0, st, row, a.Hp, a.knobs.corrupt_scale);
  return hipGetLastError();
}

// What the schedules of one call share.  A schedule takes the call's DenArgs by const reference (what the CALL decided:
// den_kernels.h) and forms what one LAUNCH needs in a copy of its own.
struct DenCall {
  int hint, gmax;
  int mask;                    // the launches this call evaluates: the caller's phase mask, less the occupancy bit of a recursion-only call
  bool corrupt;                // option debug_corrupt_row applies: written between the recursion and the occupancy launches, no overlap
  int use_ex;                  // the rows of this call were exp'd ahead (DenArgs::use_ex of its recursion / occupancy launches)
  hipStream_t st;
  const char** why;
  hipEvent_t gamma_wait, zeroed;
  SideStream* side;            // null until a schedule needs it
  bool forked = false;         // stream2 waits for the zeroed counters (and the caller's x)
  hipError_t fork_stream2() {
    if (forked) return hipSuccess;
    forked = true;
    hipError_t ef = zeroed ? hipSuccess : hipEventRecord(side->seg[0], st);
    if (ef == hipSuccess) ef = hipStreamWaitEvent(side->stream2, zeroed ? zeroed : side->seg[0], 0);
    return ef;
  }
  hipError_t launch(const DenArgs& v, hipStream_t on) const { return launch_den(v, gmax, hint, on, why); }
  hipError_t wait_gamma(hipStream_t on) const { return gamma_wait ? hipStreamWaitEvent(on, gamma_wait, 0) : hipSuccess; }
};

// a plan in the general format: den_general.hip, no overlap
hipError_t schedule_general(const DenArgs& a, const DenCall& c) {
  DenArgs v = a;
  v.phase_mask = c.mask & 1;
  hipError_t e = v.phase_mask ? launch_den_general(v, c.st) : hipSuccess;
  if (e == hipSuccess && c.corrupt && v.phase_mask) e = launch_corrupt_row(v, c.st);
  if (e == hipSuccess) e = c.wait_gamma(c.st);
  v.phase_mask = c.mask & 2;
  if (e == hipSuccess && v.phase_mask) e = launch_den_general(v, c.st);
  return e;
}

// Time segments (a.tseg, a.tburn): recursion launch over 2 B S workgroups, the check of every speculated row, the ordinary
// recursion launch as a fallback that runs only if a row did not verify, then the occupancy launch (no overlap: den_time_segments)
hipError_t schedule_time_segments(const DenArgs& a, const DenCall& c) {
  hipError_t e = hipSuccess;
  DenArgs v = a;
  if (c.mask & 1) {
    v.phase_mask = 1;
    e = c.launch(v, c.st);
    if (e == hipSuccess) e = launch_den_splice_check(v, c.st);
    v.tseg = 0; v.redo_if = 1;
    if (e == hipSuccess) e = c.launch(v, c.st);
    v.tseg = a.tseg; v.redo_if = 0;
    if (e == hipSuccess && c.corrupt) e = launch_corrupt_row(v, c.st);
  }
  if (e == hipSuccess && (c.mask & 2)) e = c.wait_gamma(c.st);
  if (e == hipSuccess && (c.mask & 2)) { v.phase_mask = 2; e = c.launch(v, c.st); }
  return e;
}

// One launch for both, or - where the occupancy launch has something to wait for - two on the caller's stream
hipError_t schedule_single(const DenArgs& a, const DenCall& c) {
  hipError_t e = hipSuccess;
  DenArgs v = a;
  v.use_ex = c.use_ex;
  if ((c.gamma_wait || c.corrupt) && (c.mask & 2)) {
    v.phase_mask = c.mask & 1;
    if (v.phase_mask) e = c.launch(v, c.st);
    if (e == hipSuccess && c.corrupt && v.phase_mask) e = launch_corrupt_row(v, c.st);
    if (e == hipSuccess) e = c.wait_gamma(c.st);
    v.phase_mask = 2;
    if (e == hipSuccess) e = c.launch(v, c.st);
  } else {
    v.phase_mask = c.mask;
    e = c.launch(v, c.st);
  }
  if (c.use_ex) {                                           // (long done: the recursions have read every row of it)
    if (e == hipSuccess) e = hipEventRecord(c.side->join2, c.side->stream2);
    if (e == hipSuccess) e = hipStreamWaitEvent(c.st, c.side->join2, 0);
  }
  return e;
}

// Streamed schedule (DenArgs::stream, den_kernels.hip: stream_take): ONE recursion launch whose workgroups report
// per-sequence progress, ONE persistent occupancy launch on the side stream - released when every recursion
// workgroup has passed T/2 (a.seg_bound[0]: nothing is computable before; the numerator has the idle CUs until then) - that
// draws rings of frames from a queue in the order in which they become computable.  No segment granularity, no exposed last
// launch: what is left when the recursions end is the last ring of every sequence.
// (The other way round - the recursion launch on the side stream, gate and occupancy launch on the caller's, so that the
// launch that ends last is followed in queue order - was measured: the wake-up of a queue that waits for another queue's
// event costs 11-19 us wherever it sits, and there the recursion paid it at the head of the step:
// profiles/r04_i_C3_step_timeline_recursion_on_side_stream.txt.)
// `finish`: den_finish_kernel is launched here, behind the recursion launch (DenArgs::occ_done)
hipError_t schedule_streamed(const DenArgs& a, DenCall& c, bool finish) {
  DenArgs v = a;
  v.use_ex = c.use_ex;
  hipError_t e = c.fork_stream2();                          // (the occupancy launch must see the zeroed counters)
  v.phase_mask = 1; v.stream = 1; v.sig_n = 1;
  if (e == hipSuccess) e = c.launch(v, c.st);
  if (e == hipSuccess) e = launch_den_gate(a.progress, den_recursion_blocks(a), a.bad, c.side->stream2);
  if (e == hipSuccess) e = c.wait_gamma(c.side->stream2);
  v.phase_mask = 2; v.stream = 3;
  v.occ_done_target = finish ? a.stream_blocks : 0;
  if (e == hipSuccess) e = c.launch(v, c.side->stream2);
  if (e == hipSuccess) e = hipEventRecord(c.side->join2, c.side->stream2);
  if (e == hipSuccess && finish) {
    DenArgs fin = a;
    fin.occ_done_target = v.occ_done_target;
    e = launch_den_finish(fin, c.st);
  }
  if (e == hipSuccess) e = hipStreamWaitEvent(c.st, c.side->join2, 0);
  return e;
}

// Gated schedule (rounds 1-2; the fallback for the two-barrier recursion and per-sequence plans, and what option
// den_segments = n asks for): ONE recursion launch; its workgroups count themselves into progress[s] when their steps
// below a.seg_bound[s] are done, and a one-wave gate kernel in front of occupancy launch s (side stream) waits for all
// of them.  (One recursion launch per segment with stream events in between - the first form of this schedule - measured
// 2 % slower and is gone: profiles/r01_*.)
hipError_t schedule_gated(const DenArgs& a, DenCall& c, int nseg) {
  DenArgs v = a;
  v.use_ex = c.use_ex;
  v.sig_n = nseg - 1;
  hipError_t e = c.fork_stream2();                          // the gates must see the zeroed counters
  v.phase_mask = 1;
  if (e == hipSuccess) e = c.launch(v, c.st);
  v.phase_mask = 2; v.gam_nseg = nseg;
  for (int s = 0; s < nseg - 1 && e == hipSuccess; s++) {
    v.gam_seg = s;
    e = launch_den_gate(a.progress + s, den_recursion_blocks(a), a.bad, c.side->stream2);
    if (e == hipSuccess && s == 0) e = c.wait_gamma(c.side->stream2);
    if (e == hipSuccess) e = c.launch(v, c.side->stream2);
  }
  // the last occupancy launch follows the recursion in stream order on the caller's stream
  v.gam_seg = nseg - 1;
  if (e == hipSuccess) e = c.wait_gamma(c.st);
  if (e == hipSuccess) e = c.launch(v, c.st);
  if (e == hipSuccess) e = hipEventRecord(c.side->join2, c.side->stream2);
  if (e == hipSuccess) e = hipStreamWaitEvent(c.st, c.side->join2, 0);
  return e;
}
}  // namespace

// `occupancy` = false: recursion only
// `gamma_wait`: event every occupancy launch has to wait for (the numerator rows it folds in), or null
// `zeroed`: an event the caller recorded on `st` behind the zeroing of the counters (the fused loss forks its numerator
// stream there), or null: recorded here.  An event record costs the caller's stream ~7 us in front of the recursion launch.
// `finish_early`: in/out - in: den_finish_kernel may be launched here (the caller has nothing else it must wait for);
// out: it was (behind the recursion launch of the streamed schedule, DenArgs::occ_done), the caller must not launch it again
// Sets what the CALL decides in `a` (den_kernels.h; the caller launches den_finish_kernel with it); a.phase_mask stays the caller's.
// (the counters the launches of a call share were zeroed with the bad count by the caller: launch_zero_words)
hipError_t run_den_launches(DenArgs& a, int hint, bool occupancy, hipStream_t st, const char** why,
                            hipEvent_t gamma_wait, hipEvent_t zeroed, bool* finish_early) {
  const bool may_finish = finish_early && *finish_early;
  if (finish_early) *finish_early = false;
  const bool both = occupancy && a.phase_mask == 3;        // a call that evaluates the recursion and the occupancy launches
  DenCall c;
  c.hint = hint; c.gmax = (a.D + 63) / 64;
  c.mask = occupancy ? a.phase_mask : (a.phase_mask & 1);
  c.corrupt = a.knobs.corrupt_what == 1 && a.knobs.corrupt_b < a.B && a.knobs.corrupt_t < a.T;
  c.use_ex = 0;
  c.st = st; c.why = why; c.gamma_wait = gamma_wait; c.zeroed = zeroed; c.side = nullptr;
  den_decide_family(a, hint);
  // the invariant check (DenArgs::tot_a) needs the recursions and the occupancy launches of ONE call
  a.check = both ? 1 : 0;
  if (hint == PYCHAIN_HIP_HINT_GENERAL) return schedule_general(a, c);
  // a "pdf by state" plan whose recursions emit the occupancies of their own second halves themselves (DenArgs::xf): a call of the
  // denominator alone that evaluates both launches; the occupancy launch then follows the recursions and handles the bands around
  // the middles (each direction waits for rows of the other: every workgroup of the launch must be resident at once)
  a.xf = (a.sg && both && !c.corrupt && zeroed == nullptr && 2 * a.B <= device_cu_count() && den_xf_eligible(a, hint)) ? den_xf_band() : 0;
  const int nseg = (both && !a.check_all && !c.corrupt && !a.xf) ? den_segments(a) : 1;
  // Rows exp'd ahead of the lazy recursions by a launch of its own on the side stream (DenArgs::ex), whichever schedule
  // follows (option den_dma = 2: the recursions clamp / exp their rows themselves, as they do for short sequences, rows
  // that are not a multiple of four pdfs and callers that hand in exp'd rows) - in a call of the denominator alone and a
  // workspace that holds the buffer.  NOT in the fused loss (`zeroed`): there the CUs the recursions leave idle are booked - the
  // numerator until T/2, the occupancy launch from there to the end - and the launch's registers and HBM traffic held the
  // numerator back by 1 ms (C3: 3.02 -> 3.31 ms per step with it, although the recursion itself ran 4 % faster:
  // profiles/r04_u_C3_step_timeline_rows_exp_ahead_in_the_fused_step.txt).
  const bool exp_ahead = a.ex != nullptr && zeroed == nullptr && den_would_exp_rows_ahead(a) && (a.phase_mask & 1) != 0;
  // (den_would_exp_rows_ahead: false where den_time_segments says > 1)
  const int tseg = exp_ahead ? 1 : den_time_segments(a, zeroed != nullptr);
  if (exp_ahead || (tseg <= 1 && nseg > 1)) {
    c.side = side_streams_for(st);
    if (!c.side) { *why = "cannot create the side streams"; return hipErrorInvalidValue; }
  }
  if (exp_ahead) {
    hipError_t e = c.fork_stream2();
    den_exp_rows_shape(a, device_cu_count(), &a.ex_nr, &a.ex_q);
    if (e == hipSuccess) e = launch_den_exp_rows(a, c.side->stream2);
    if (e != hipSuccess) return e;
    c.use_ex = 1;
  }
  if (tseg > 1) {
    if (c.mask & 1) { a.tseg = tseg; a.tburn = a.knobs.den_tburn; }   // (stay set for den_finish_kernel: an inner segment's NaN report)
    return schedule_time_segments(a, c);
  }
  if (nseg <= 1) return schedule_single(a, c);
  // Frame t becomes computable after max(t, L-1-t) recursion steps, i.e. nothing before T/2 and
  // then ever faster: segment ends at T/2, 3T/4, 7T/8, ... so every occupancy launch but the
  // last overlaps the next recursion segment and the last one holds ~2^-(nseg-1) of the frames.
  for (int s = 0; s < nseg; s++) {
    const double frac = s == nseg - 1 ? 1.0 : 1.0 - 1.0 / (double)(2 << s);
    a.seg_bound[s] = s == nseg - 1 ? a.T : ((int)(frac * a.T) + 31) / 32 * 32;
  }
  if (a.knobs.den_segments != 0 || !den_stream_eligible(a, c.gmax, hint)) return schedule_gated(a, c, nseg);
  a.stream_blocks = device_cu_count();
  a.seg_bound[0] = std::min(a.T, (a.T / 2 + 31) / 32 * 32);
  const hipError_t e = schedule_streamed(a, c, may_finish);
  if (e == hipSuccess && may_finish) *finish_early = true;
  return e;
}

// ... and, behind all of them on the caller's stream, den_finish_kernel: objf from the per-frame totals and
// the reference's invariant check (DenArgs::tot_a)
hipError_t run_den(DenArgs& a, int hint, bool occupancy, hipStream_t st, const char** why, hipEvent_t gamma_wait) {
  bool finished = gamma_wait == nullptr;                 // (a caller with an event of its own launches den_finish_kernel itself)
  hipError_t e = run_den_launches(a, hint, occupancy, st, why, gamma_wait, nullptr, &finished);
  if (e == hipSuccess && (a.phase_mask & 1) && !finished) e = launch_den_finish(a, st);   // objf (+ the check) from the stored totals
  return e;
}

}  // namespace pychain_hip
