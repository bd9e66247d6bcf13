// smbr_device.h - the device code of the reference-layout recursions, ONE copy for the three translation units that run them
// (smbr.hip: sMBR with a frame in LDS; smbr_general.hip: the general sMBR kernels, §3.28; arc_counts.hip:
// expected arc counts, §3.29): the workgroup shapes, the block sum, the ownership of a frame's target entries, the class table, the
// staging of a network-output row, and
//   recursion       the persistent workgroup of a (sequence, direction): with or without the accuracy-weighted pair, pdf-level or
//                   by class, over any FrameStore
//   smbr_grad_frame one frame of the sMBR gradient, pdf-level or by class, over FrameLds or FrameGlobal
//   smbr_close      a sequence's closing diagnostic and verdict
// The kernels of the three units are wrappers that lay out their storage and call these.  The general kernels give the bits of
// the LDS kernels, and arc counts the alpha' and beta' of sMBR, BECAUSE these are one copy: the same partial sums in the same
// order, the same owner of every entry.  Include it behind `#pragma clang fp contract(off)`, as the three units do.
#ifndef PYCHAIN_HIP_SMBR_DEVICE_H_
#define PYCHAIN_HIP_SMBR_DEVICE_H_

#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_utils.h"
#include "row_access.h"
#include "smbr.h"

namespace pychain_hip {
namespace {

constexpr int kSmNT = 1024;                 // recursion workgroup: 16 waves
constexpr int kSmGNT = 512;                 // gradient workgroup
constexpr int kSmFrames = 8;                // frames of one gradient workgroup
constexpr int kSmXR = 4;                    // elements of the next row a recursion thread holds in registers across the arc loop
constexpr int kSmRed = 64;                  // floats of reduction scratch
static_assert(48 + kSmGNT / 64 <= kSmRed, "smbr_grad_frame sums the row mean over red[48 ..], behind block_sum3's 3 x 16");
constexpr size_t kSmStaticLds = 256;        // what the recursion kernel holds beside its dynamic LDS (the closing vote)

// ---- where a frame lives ----------------------------------------------------------------------------------------------------------
// a float written by another thread of this workgroup to global memory before the last barrier: read around the (non-coherent)
// vector L1, as den_general.hip reads it
__device__ __forceinline__ float load_fresh(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The storage of a frame.  ROWS_LDS: the D-rows (x, x A; the gradient's x q0, x (q1 + a q0)) and the class table lie in LDS, else in
// a scratch row of the workspace.  VEC_LDS: the state vectors lie in LDS - double-buffered in the recursion, staged per frame in the
// gradient -, else they are read where the trajectories hold them, and a recursion keeps its raw sums in the row it is making.
// What another thread wrote before the last barrier is read by row() / vec(); a writer calls publish() ahead of that barrier.
// Index: the arithmetic of an arc's place in the graph arrays - int where a frame fits LDS, as those kernels always had it (their
// address arithmetic is on the arc loop's way), 64 bits in the general kernels, which take any graph the int32 layout holds.
template <bool ROWS_LDS, bool VEC_LDS>
struct FrameStore {
  static constexpr bool kVecLds = VEC_LDS;
  using Index = std::conditional_t<ROWS_LDS, int, size_t>;
  static __device__ __forceinline__ float row(const float* p) { if constexpr (ROWS_LDS) return *p; else return load_fresh(p); }
  static __device__ __forceinline__ float vec(const float* p) { if constexpr (VEC_LDS) return *p; else return load_fresh(p); }
  static __device__ __forceinline__ void publish() { if constexpr (!ROWS_LDS) __threadfence(); }
};
using FrameLds = FrameStore<true, true>;         // smbr.hip, arc_counts.hip
using FrameRows = FrameStore<false, true>;       // smbr_general.hip: "rows"
using FrameGlobal = FrameStore<false, false>;    // smbr_general.hip: "global", and its gradient

// up to three sums over the workgroup, every thread gets the totals; `red` (3 x 16 floats) is free again behind the NEXT barrier
template <int NT>
__device__ __forceinline__ void block_sum3(float& s0, float& s1, float& s2, float* red, int tid) {
  s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
  if ((tid & 63) == 0) { red[tid >> 6] = s0; red[16 + (tid >> 6)] = s1; red[32 + (tid >> 6)] = s2; }
  __syncthreads();
  s0 = s1 = s2 = 0.f;
  for (int w = 0; w < NT / 64; w++) { s0 += red[w]; s1 += red[16 + w]; s2 += red[32 + w]; }     // (same order in every thread)
}

// Entry k of a frame (pd, pr: its Kt entries): true where this thread owns it, with (pdf, summed q).  An entry is handled where
// its pdf occurs first in the frame, q summed in ascending k, so a repeated pdf has one owner and nothing is atomic.
__device__ __forceinline__ bool owned_entry(const int32_t* pd, const float* pr, int k, int Kt, int D, int& d, float& q) {
  d = pd[k];
  if (d < 0 || d >= D) return false;
  for (int j = 0; j < k; j++)
    if (pd[j] == d) return false;
  q = pr[k];
  for (int j = k + 1; j < Kt; j++)
    if (pd[j] == d) q += pr[j];
  return true;
}
// x A of a frame over its zeroed companion row
template <class S>
__device__ __forceinline__ void scatter_entries(const int32_t* pd, const float* pr, int Kt, int D, int tid, int nt, const float* xrow, float* xacc) {
  int d;
  float q;
  for (int k = tid; k < Kt; k += nt)
    if (owned_entry(pd, pr, k, Kt, D, d, q)) xacc[d] = S::row(xrow + d) * q;
}

// ---- accuracy by class (§3.27) ----------------------------------------------------------------------------------------------------
// the class of a target id, -1 where it adds nothing: padding, a pdf >= D, a class >= C
__device__ __forceinline__ int entry_class(const SmbrClasses& c, int id, int D) {
  if (id < 0) return -1;
  if (c.targets_are_classes) return id < c.C ? id : -1;
  return id < D ? c.cls[id] : -1;
}
// Acls(t, .) of a frame into `acl` [C]: thread tid, tid + nt, ... sums the q of its class in ascending k - one owner, no atomics
__device__ __forceinline__ void class_table(const SmbrClasses& c, const int32_t* pd, const float* pr, int Kt, int D, int tid, int nt, float* acl) {
  for (int cc = tid; cc < c.C; cc += nt) {
    float q = 0.f;
    for (int k = 0; k < Kt; k++)
      if (entry_class(c, pd[k], D) == cc) q += pr[k];
    acl[cc] = q;
  }
}

// ---- the frame's row ------------------------------------------------------------------------------------------------------------
// row t of the sequence into `lds` (LDS, or a scratch row of the general kernels) as exp(clamp(.)); elements tid + i * NT,
// i < kSmXR, come from `held` (loaded before the arc loop)
template <int XH>
__device__ __forceinline__ void hold_row(const void* x, size_t row, int D, int tid, float (&held)[kSmXR]) {
#pragma unroll
  for (int i = 0; i < kSmXR; i++) {
    const int n = tid + i * kSmNT;
    held[i] = n < D ? row_load1<XH>(x, row + n) : 0.f;
  }
}
template <int XH>
__device__ __forceinline__ bool put_row(const void* x, size_t row, int D, int tid, const float (&held)[kSmXR], float* lds) {
  bool nan = false;
#pragma unroll
  for (int i = 0; i < kSmXR; i++) {
    const int n = tid + i * kSmNT;
    if (n < D) { nan = nan || held[i] != held[i]; lds[n] = clamp_exp(held[i], kXExpClamp); }
  }
  for (int n = tid + kSmXR * kSmNT; n < D; n += kSmNT) {       // (rows of more than 4096 pdfs)
    const float r = row_load1<XH>(x, row + n);
    nan = nan || r != r;
    lds[n] = clamp_exp(r, kXExpClamp);
  }
  return nan;
}
// x A of the elements put_row stored, by class: xacc[n] = xrow[n] * acl[cls[n]] - the row element is the thread's own, the table
// other threads'; `hc`: cls of the elements held in registers, those beyond are loaded again
template <class S>
__device__ __forceinline__ void class_row(const int32_t* cls, const int (&hc)[kSmXR], int D, int tid, const float* acl, const float* xrow, float* xacc) {
#pragma unroll
  for (int i = 0; i < kSmXR; i++) {
    const int n = tid + i * kSmNT;
    if (n < D) xacc[n] = S::row(xrow + n) * S::row(acl + hc[i]);
  }
  for (int n = tid + kSmXR * kSmNT; n < D; n += kSmNT) xacc[n] = S::row(xrow + n) * S::row(acl + cls[n]);
}

// ---- the recursion ----------------------------------------------------------------------------------------------------------------
// What a recursion workgroup reads and writes, filled at the top of each kernel from its own argument struct (SmbrArgs, or the
// ArcArgs of arc_counts.hip), and where the kernel laid out the frame's storage.  Without the weighted pair ab, bb, the targets,
// frame_acc, vec1, xacc and acl stay null.
struct RecArgs {
  const SmbrGraph& g;
  const float *pf, *pb;                  // [K] arc probabilities in the forward / in the backward order
  const void* x; const int64_t* lengths;
  const int32_t* pdfs; const float* probs; const float* frame_acc;
  float coef;
  float *al, *ab, *be, *bb;              // the trajectory stores [B][T+1][H]
  float *tot_a, *tot_b;                  // [B][T+1]
  int32_t* seq_bad;                      // [B]
  int T, D, Kt;
  float *vec0, *vec1;                    // [2][H] alpha' / beta', alpha-bar' / beta-bar' (S::kVecLds)
  float *xrow, *xacc;                    // [2][D] x, x * A
  float* acl;                            // [C] Acls of the frame whose companion row is made next (CLS)
  float* red;                            // [kSmRed], LDS
};
// ... of an sMBR call, the storage left to the kernel
__device__ __forceinline__ RecArgs smbr_rec_args(const SmbrArgs& a) {
  RecArgs r{a.g};
  r.pf = a.g.fp; r.pb = a.g.bp; r.x = a.x; r.lengths = a.lengths; r.pdfs = a.pdfs; r.probs = a.probs; r.frame_acc = a.frame_acc;
  r.coef = a.coef; r.al = a.al; r.ab = a.ab; r.be = a.be; r.bb = a.bb; r.tot_a = a.tot_a; r.tot_b = a.tot_b; r.seq_bad = a.seq_bad;
  r.T = a.T; r.D = a.D; r.Kt = a.Kt;
  return r;
}

// One persistent workgroup of kSmNT threads per (sequence, direction), carrying alpha' (FWD) or beta' - with PAIR also the
// accuracy-weighted alpha-bar' or beta-bar' - double-buffered, with the frame's row x = exp(clamp(y)) and, with PAIR, its companion
// xa(n) = x(n) A(t,n); both rows are made a frame ahead.  Arcs come from global memory in the reference layout (by destination
// forwards, by source backwards); a thread owns states tid, tid + 1024, ...  The accuracies are CENTRED, a(t,n) = A(t,n) - e(t):
// the source term of a frame is sum alpha' p xa - e(t) * (the first-order sum), so that only the frame's K entries need a row.
// alpha-bar and beta-bar take the per-frame normalisers of alpha and beta.
// CLS: the accuracy by class (§3.27) - `c` is read, and the companion row is dense: made from the next row and the next frame's
// table (written before the arc loop) in the slot where the pdf-level form scatters its K entries.
// No workgroup waits for another; every loop is bounded by L_b <= T.
template <int XH, bool FWD, bool CLS, bool PAIR, class S>
__device__ __forceinline__ void recursion(const RecArgs& r, const SmbrClasses& c, int b) {
  static_assert(PAIR || !CLS, "the class table serves the weighted pair");
  using Index = typename S::Index;
  const int tid = threadIdx.x;
  const SmbrGraph& g = r.g;
  const int H = g.H, D = r.D, T = r.T, Kt = r.Kt;
  const int L = seq_len(r.lengths, b, T);
  float *const vec0 = r.vec0, *const vec1 = r.vec1, *const xrow = r.xrow, *const xacc = r.xacc, *const acl = r.acl, *const red = r.red;
  int hc[kSmXR];
  if constexpr (CLS) {
#pragma unroll
    for (int i = 0; i < kSmXR; i++) hc[i] = tid + i * kSmNT < D ? c.cls[tid + i * kSmNT] : 0;
  }
  const size_t seq_rows = (size_t)b * (T + 1);
  float* const st0 = (FWD ? r.al : r.be) + seq_rows * H;
  float* const st1 = PAIR ? (FWD ? r.ab : r.bb) + seq_rows * H : nullptr;
  float* const totv = (FWD ? r.tot_a : r.tot_b) + seq_rows;
  const int32_t* const idx = FWD ? g.bi : g.fi;                // forwards: the arcs ENTERING a state; backwards: those leaving it
  const int32_t* const arc = FWD ? g.bt : g.ft;
  const float* const pr = FWD ? r.pb : r.pf;
  const float coef = r.coef;
  const size_t xseq = (size_t)b * T * D, fseq = (size_t)b * T;
  bool bad = false, nan = false;

  // the first row: alpha'(0) from the initial, beta'(L) from the final probabilities; the weighted vector starts at zero
  {
    const float* start = FWD ? g.init : g.fin;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int i = tid; i < H; i += kSmNT) { s0 += start[i]; s1 += start[i] * g.leaky[i]; }
    block_sum3<kSmNT>(s0, s1, s2, red, tid);
    const float inv = 1.f / s0;
    if (!(s0 > 0.f) || !(inv > 0.f) || !(inv - inv == 0.f)) bad = true;
    const int r0 = FWD ? 0 : L;
    if (tid == 0) totv[r0] = s0;
    for (int i = tid; i < H; i += kSmNT) {
      const float v = FWD ? start[i] * inv + coef * g.leaky[i] : (start[i] + coef * s1) * inv;
      if constexpr (S::kVecLds) { vec0[i] = v; if constexpr (PAIR) vec1[i] = 0.f; }
      st0[(size_t)r0 * H + i] = v;
      if constexpr (PAIR) st1[(size_t)r0 * H + i] = 0.f;
    }
    const int t0 = FWD ? 0 : L - 1;
    float held[kSmXR];
    hold_row<XH>(r.x, xseq + (size_t)t0 * D, D, tid, held);
    nan = put_row<XH>(r.x, xseq + (size_t)t0 * D, D, tid, held, xrow) || nan;
    if constexpr (PAIR) {
      const int32_t* pd = r.pdfs + (fseq + t0) * Kt;
      const float* pq = r.probs + (fseq + t0) * Kt;
      if constexpr (CLS) class_table(c, pd, pq, Kt, D, tid, kSmNT, acl);
      else for (int n = tid; n < D; n += kSmNT) xacc[n] = 0.f;
      S::publish();
      __syncthreads();
      if constexpr (CLS) class_row<S>(c.cls, hc, D, tid, acl, xrow, xacc);
      else scatter_entries<S>(pd, pq, Kt, D, tid, kSmNT, xrow, xacc);
    }
    S::publish();
    __syncthreads();
  }
  // frame j: forwards alpha'(t+1) from alpha'(t) and x(t), t = j; backwards beta'(t) from beta'(t+1) and x(t), t = L-1-j
  for (int j = 0; j < L; j++) {
    const int p = j & 1;
    const int t = FWD ? j : L - 1 - j, tn = FWD ? t + 1 : t - 1;
    const bool more = j + 1 < L;
    const int rn = FWD ? t + 1 : t, rp = FWD ? t : t + 1;                      // the row made, the row it is made from
    const float* v0 = S::kVecLds ? vec0 + (size_t)p * H : st0 + (size_t)rp * H;
    const float* v1 = !PAIR ? nullptr : S::kVecLds ? vec1 + (size_t)p * H : st1 + (size_t)rp * H;
    float* w0 = S::kVecLds ? vec0 + (size_t)(1 - p) * H : st0 + (size_t)rn * H;      // (!kVecLds: raw sums wait in the row's own slot)
    float* w1 = !PAIR ? nullptr : S::kVecLds ? vec1 + (size_t)(1 - p) * H : st1 + (size_t)rn * H;
    const float* xr = xrow + (size_t)p * D;
    const float* xa = PAIR ? xacc + (size_t)p * D : nullptr;
    float* xrn = xrow + (size_t)(1 - p) * D;
    float* xan = PAIR ? xacc + (size_t)(1 - p) * D : nullptr;
    float held[kSmXR];
    if (more) hold_row<XH>(r.x, xseq + (size_t)tn * D, D, tid, held);          // the next frame's row: in flight over the arc loop
    if constexpr (CLS) {                                                       // (the table's readers are behind the last barrier)
      if (more) class_table(c, r.pdfs + (fseq + tn) * Kt, r.probs + (fseq + tn) * Kt, Kt, D, tid, kSmNT, acl);
    } else if constexpr (PAIR) {
      for (int n = tid; n < D; n += kSmNT) xan[n] = 0.f;
    }
    const float e_t = PAIR ? r.frame_acc[fseq + t] : 0.f;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int i = tid; i < H; i += kSmNT) {
      float acc0 = 0.f, acc1 = 0.f;
      const int k1 = idx[2 * (Index)i + 1];
      for (int k = idx[2 * (Index)i]; k < k1; k++) {
        const int other = arc[3 * (Index)k + (FWD ? 0 : 1)], n = arc[3 * (Index)k + 2];
        const float w = pr[k], u0 = S::vec(v0 + other), u1 = PAIR ? S::vec(v1 + other) : 0.f;
        const float xx = S::row(xr + n), xq = PAIR ? S::row(xa + n) : 0.f;
        const float wu = w * u0;
        acc0 += wu * xx;
        if constexpr (PAIR) acc1 += (w * u1) * xx + wu * xq;
      }
      if constexpr (PAIR) acc1 -= e_t * acc0;                                  // the centring: a(t,n) = A(t,n) - e(t)
      w0[i] = acc0;                                                            // raw, finished below by the thread that wrote them
      if constexpr (PAIR) w1[i] = acc1;
      s0 += acc0;
      if (FWD) { if constexpr (PAIR) s1 += acc1; }
      else { s1 += acc0 * g.leaky[i]; if constexpr (PAIR) s2 += acc1 * g.leaky[i]; }
    }
    if (more) nan = put_row<XH>(r.x, xseq + (size_t)tn * D, D, tid, held, xrn) || nan;
    S::publish();                                                              // (the next row, its zeroed companion, the table)
    block_sum3<kSmNT>(s0, s1, s2, red, tid);                                   // (its barrier: the next rows are whole)
    if constexpr (CLS) {
      if (more) class_row<S>(c.cls, hc, D, tid, acl, xrn, xan);
    } else if constexpr (PAIR) {
      if (more) scatter_entries<S>(r.pdfs + (fseq + tn) * Kt, r.probs + (fseq + tn) * Kt, Kt, D, tid, kSmNT, xrn, xan);
    }
    const float inv = 1.f / s0;
    if (!(s0 > 0.f) || !(inv > 0.f) || !(inv - inv == 0.f)) bad = true;
    if (tid == 0) totv[rn] = s0;
    float* const o0 = st0 + (size_t)rn * H;
    float* const o1 = PAIR ? st1 + (size_t)rn * H : nullptr;
    for (int i = tid; i < H; i += kSmNT) {
      float c0, c1 = 0.f;
      if (FWD) {
        const float lk = coef * g.leaky[i];
        c0 = w0[i] * inv + lk;                                                 // (the normalised alpha sums to one)
        if constexpr (PAIR) c1 = (w1[i] + lk * s1) * inv;
      } else {
        c0 = (w0[i] + coef * s1) * inv;
        if constexpr (PAIR) c1 = (w1[i] + coef * s2) * inv;
      }
      if constexpr (S::kVecLds) { w0[i] = c0; if constexpr (PAIR) w1[i] = c1; }
      o0[i] = c0;
      if constexpr (PAIR) o1[i] = c1;
    }
    S::publish();                                                              // (the companion row; !kVecLds: the state rows)
    __syncthreads();
  }
  // a NaN in a live row of x (the clamp turns it into exp(-30): watched here, by the forward workgroup), a total that is not
  // positive and finite: the sequence is bad.  (Both workgroups of a sequence may store the same 1.)
  if (__syncthreads_or((bad || (FWD && nan)) ? 1 : 0) && tid == 0) r.seq_bad[b] = 1;
}

// ---- the verdict ----------------------------------------------------------------------------------------------------------------
// The sequence went bad: its E_b becomes NaN and it is counted ONCE, by whichever workgroup of the gradient launch finds it first
// (seq_bad[B + b]: claimed by an integer compare-and-swap; the same values whoever wins).
__device__ __forceinline__ void smbr_condemn(const SmbrArgs& a, int b) {
  if (atomicCAS(a.seq_bad + a.B + b, 0, 1) == 0) {
    a.acc_per_seq[b] = __builtin_nan("");
    atomicAdd(a.bad_count, 1);                                                 // (an integer count)
  }
}
// closes a sequence, by the workgroup that has its first frames: the diagnostic sum_j alpha-bar'(L,j) final(j) / sum_j alpha'(L,j)
// final(j), and the sequence's verdict
__device__ __forceinline__ void smbr_close(const SmbrArgs& a, int b, int L, float* red) {
  const int tid = threadIdx.x, H = a.g.H;
  const size_t rL = ((size_t)b * (a.T + 1) + L) * H;
  float c0 = 0.f, c1 = 0.f, none = 0.f;
  for (int i = tid; i < H; i += kSmGNT) { c0 += a.al[rL + i] * a.g.fin[i]; c1 += a.ab[rL + i] * a.g.fin[i]; }
  block_sum3<kSmGNT>(c0, c1, none, red, tid);
  if (tid == 0) {
    const bool bad = a.seq_bad[b] != 0 || !(c0 > 0.f);                         // what the recursions found
    a.closing[b] = bad ? __builtin_nanf("") : c1 / c0;
    if (bad) smbr_condemn(a, b);
  }
}

// ---- the gradient -----------------------------------------------------------------------------------------------------------------
// Frame t of sequence b (of L frames), by a workgroup of kSmGNT threads: a thread owns pdfs tid, tid + 512, ... and walks that pdf's arcs through
// the caller's by-pdf order:
//   q0 = sum p alpha' beta',  q1 = sum p (alpha-bar' beta' + alpha' beta-bar')
//   v = x (q1 + a q0),  grad = s (v - eps x q0) / sum_m x(m) q0(m),  eps = sum_m v(m) / sum_m x(m) q0(m)
// (the row centred by its own mean: §3.26, "the residue").  The frame's normalisers cancel in the quotient, as in
// den_general_gamma_kernel.  The four state rows alpha'(t), alpha-bar'(t), beta'(t+1), beta-bar'(t+1) are staged in `stage` [4][H]
// (S::kVecLds) or read where the recursion launch left them; gq, gv [D] and acl [C] lie where S says.
// CLS (§3.27): the frame's table is made first and every carried pdf takes its class's credit in the pass that forms it, where the
// pdf-level form adds the K owned entries behind the reduction.
template <int XH, bool CLS, class S>
__device__ __forceinline__ void smbr_grad_frame(const SmbrArgs& a, const SmbrClasses& c, int b, int t, int L, float gscale,
                                                float* stage, float* gq, float* gv, float* acl, float* red) {
  const int tid = threadIdx.x;
  const SmbrGraph& g = a.g;
  const int H = g.H, D = a.D, T = a.T, Kt = a.Kt;
  const size_t row = ((size_t)b * T + t) * D;
  if (t >= L) {                                                               // padding: exact zeros
    for (int n = tid; n < D; n += kSmGNT) row_store1<XH>(a.grad, row + n, 0.f);
    return;
  }
  const size_t r0 = ((size_t)b * (T + 1) + t) * H, r1 = r0 + H;
  const float* const sa = S::kVecLds ? stage : a.al + r0;                      // alpha'(t)
  const float* const sab = S::kVecLds ? stage + H : a.ab + r0;                 // alpha-bar'(t)
  const float* const sb = S::kVecLds ? stage + 2 * (size_t)H : a.be + r1;      // beta'(t+1)
  const float* const sbb = S::kVecLds ? stage + 3 * (size_t)H : a.bb + r1;     // beta-bar'(t+1)
  const int32_t* pd = a.pdfs + ((size_t)b * T + t) * Kt;
  const float* pq = a.probs + ((size_t)b * T + t) * Kt;
  if constexpr (S::kVecLds)
    for (int i = tid; i < H; i += kSmGNT) {
      stage[i] = a.al[r0 + i]; stage[H + i] = a.ab[r0 + i]; stage[2 * (size_t)H + i] = a.be[r1 + i]; stage[3 * (size_t)H + i] = a.bb[r1 + i];
    }
  if constexpr (CLS) { class_table(c, pd, pq, Kt, D, tid, kSmGNT, acl); S::publish(); }
  if constexpr (S::kVecLds || CLS) __syncthreads();
  const float e_t = a.frame_acc[(size_t)b * T + t];
  float part = 0.f, mean = 0.f, none = 0.f;
  for (int n = tid; n < D; n += kSmGNT) {
    const int k0 = g.pidx[n], k1 = g.pidx[n + 1];
    float q0 = 0.f, q1 = 0.f;
    for (int k = k0; k < k1; k++) {
      const int id = g.parc[k];
      const int src = g.ft[3 * (typename S::Index)id], dst = g.ft[3 * (typename S::Index)id + 1];
      const float w = g.fp[id];
      const float wa = w * sa[src];
      q0 += wa * sb[dst];
      q1 += (w * sab[src]) * sb[dst] + wa * sbb[dst];
    }
    float v0 = 0.f, v1 = 0.f;
    if (k0 != k1) {                                                            // a pdf no arc carries: its x is not read
      const float xx = clamp_exp(row_load1<XH>(a.x, row + n), kXExpClamp);
      v0 = xx * q0;
      v1 = xx * (q1 - e_t * q0);
      if constexpr (CLS) v1 += S::row(acl + c.cls[n]) * v0;                    // (+ A x q0: the thread's own element)
    }
    gq[n] = v0; gv[n] = v1;
    part += v0;
    if constexpr (CLS) mean += v1;                                             // (by class the row's mean rides in the block sum)
  }
  if constexpr (!CLS) S::publish();                                            // (the entries' owners read other threads' elements)
  block_sum3<kSmGNT>(part, mean, none, red, tid);
  if constexpr (!CLS) {
    int d;
    float q;
    for (int k = tid; k < Kt; k += kSmGNT)
      if (owned_entry(pd, pq, k, Kt, D, d, q)) gv[d] = S::row(gv + d) + q * S::row(gq + d);
    S::publish();
    __syncthreads();
    // The row's mean: a second sum, over the FINISHED elements.  (Summing x (q1 - e q0) in the first block sum and the owners'
    // A x q0 beside it gives the same mean in exact arithmetic, but at a pdf with gamma near one the two halves are each as large
    // as the divisor and cancel: the mean must carry the rounding its elements carry, or it spreads 1e-7 of gamma over the row.)
    // Its scratch is red[48 ..], which block_sum3 leaves alone - slower waves may still read red[0 .. 47].
    mean = 0.f;
    for (int n = tid; n < D; n += kSmGNT) mean += S::row(gv + n);
    mean = wave_sum(mean);
    if ((tid & 63) == 0) red[48 + (tid >> 6)] = mean;
    __syncthreads();
    mean = 0.f;
    for (int w = 0; w < kSmGNT / 64; w++) mean += red[48 + w];                 // (same order in every thread)
  }
  const float sc = gscale / part, inv = 1.f / part;
  if ((!(part > 0.f) || !(inv - inv == 0.f)) && tid == 0) smbr_condemn(a, b);  // (the host twin's check of the same divisor)
  // The row is centred by its own mean: sum_n x (q1 + a q0) is zero but for the rounding of e(t) - the occupancies are another
  // kernel's, in fp32 -, and that residue enters alpha-bar and beta-bar at every frame and stays: uncentred, the row carries
  // gamma(t,n) times the residue accumulated over the sequence (`closing` is that sum; DESIGN.md §3.26, "The residue").
  const float eps = mean * inv;
  for (int n = tid; n < D; n += kSmGNT) {
    const bool carried = g.pidx[n] != g.pidx[n + 1];
    row_store1<XH>(a.grad, row + n, carried ? (S::row(gv + n) - eps * S::row(gq + n)) * sc : 0.f);
  }
  __syncthreads();                                                             // (the rows and red are free for the next frame)
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------
// a kernel with `lds` bytes of dynamic LDS: the attribute that admits more than 64 KiB, the launch, its error
template <class... P, class... A>
hipError_t launch_with_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  return hipGetLastError();
}
// f(integral_constant<int, XH>) for the row dtype xh: kXF32, kXBf16 or kXF16 (the caller checked)
template <class F>
hipError_t by_row_dtype(int xh, F&& f) {
  if (xh == kXF32) return f(std::integral_constant<int, kXF32>());
  if (xh == kXBf16) return f(std::integral_constant<int, kXBf16>());
  return f(std::integral_constant<int, kXF16>());
}

}  // namespace
}  // namespace pychain_hip
#endif
