// smbr.hip - lattice-free sMBR (include/pychain_hip.h: pychain_hip_smbr_*): the expected frame accuracy of the
// denominator's path distribution against a reference given as sparse per-frame targets, E = sum_t sum_n gamma(t,n) A(t,n), and
// its gradient dE/dy(t,n) = gamma(t,n) (E[score | pdf n at t] - E).  The gradient is a covariance under the path distribution:
// beside alpha' and beta' it needs the accuracy-weighted pair alpha-bar', beta-bar', which no other kernel of the library forms.
//
//   smbr_frame_acc_kernel    e(b,t) = sum_k q_k gamma(b,t,pdf_k) from the occupancies of the ordinary denominator call, and
//                            E_b = sum_t e(b,t) in fp64.  One workgroup per sequence, a thread per frame.
//   smbr_recursion_kernel    2B persistent workgroups, one per (sequence, direction), each carrying (alpha', alpha-bar') or
//                            (beta', beta-bar') in LDS, double-buffered, with the frame's row x = exp(clamp(y)) and its sparse
//                            companion xa(n) = x(n) A(t,n); both rows are made a frame ahead.  Arcs come from global memory in the
//                            reference layout (by destination forwards, by source backwards); a thread owns states tid, tid + 1024,
//                            ...  The accuracies are CENTRED, a(t,n) = A(t,n) - e(t): the source term of a frame is
//                            sum alpha' p xa - e(t) * (the first-order sum), so that only the frame's K entries need a row.
//                            alpha-bar and beta-bar take the per-frame normalisers of alpha and beta.  No workgroup waits for
//                            another; every loop is bounded by L_b <= T.
//   smbr_grad_kernel         time-parallel over (sequence, block of frames): the four state rows of a frame in LDS, a thread owns
//                            pdfs tid, tid + 512, ... and walks that pdf's arcs through the caller's by-pdf order:
//                              q0 = sum p alpha' beta',  q1 = sum p (alpha-bar' beta' + alpha' beta-bar')
//                              v = x (q1 + a q0),  grad = s (v - eps x q0) / sum_m x(m) q0(m),  eps = sum_m v(m) / sum_m x(m) q0(m)
//                            (the row centred by its own mean: §3.26, "the residue")
//                            The frame's normalisers cancel in the quotient, as in den_general_gamma_kernel.
//
// The same with the accuracy by CLASS (pychain_hip_smbr_*_classes): A(t,n) = Acls(t, cls[n]) for a map cls from
// pdf to class, Acls(t,c) = the sum of the frame's q_k whose class is c.  A row of A is dense then, which none of the three
// kernels above can take, so each has a counterpart; the pdf-level kernels keep their code.
//   smbr_class_frame_acc_kernel   a dense pass over gamma: a wave per frame on a grid over (frames, B), the frame's entries merged
//                                 into distinct classes first, fp64 sums in a fixed order; smbr_class_seq_acc_kernel sums E_b
//   smbr_class_recursion_kernel   smbr_recursion with CLS: one table Acls(t, .) in LDS, written for the next frame before the arc
//                                 loop; the dense companion row x A is made behind the reduction's barrier, where the pdf-level
//                                 form scatters its K entries.  No barrier more, the arc loop unchanged.
//   smbr_class_grad_kernel        the frame's table made beside the state rows; every carried pdf takes its class's credit; the
//                                 row is centred by its own mean (the residue of e(t)'s rounding, which a dense A would spread)
// Nothing is atomic but integer counters and flags; every sum has a fixed order, so a call gives the same bits every time.  All of
// this unit's device code, the helpers of the project's headers included, is compiled with contraction off: the 2-byte forms then compute what the fp32 form computes on the up-cast input.
//
// These kernels keep a frame in LDS and the two entry points that launch only them refuse what does not fit.  The general kernels
// (smbr_general.hip) take any graph and tree with the same bits; they share this unit's argument checks, workspace
// layout and entry-point code (pychain_hip_smbr_forward_backward_general, pychain_hip_smbr_form, below) and the device helpers of
// smbr_device.h.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#pragma clang fp contract(off)      // ahead of the project's headers: their inline helpers (clamp_exp, the row loads) are under it too

#include "../../include/pychain_hip.h"
#include "call_args.h"
#include "common.h"
#include "row_access.h"
#include "smbr.h"
#include "smbr_device.h"

namespace pychain_hip {
namespace {

// (the workgroup shapes, block_sum3, owned_entry, scatter_entries, entry_class, class_table, hold_row, put_row and smbr_condemn:
// smbr_device.h, shared with the general kernels of smbr_general.hip)
constexpr int kSmAccNT = 256;

// ---- stage 1: frame accuracies ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSmAccNT) void smbr_frame_acc_kernel(const SmbrAccArgs a) {
  __shared__ double red[kSmAccNT / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int L = seq_len(a.lengths, b, a.T);
  double sum = 0.0;
  int bad = 0;
  for (int t = tid; t < L; t += kSmAccNT) {
    const size_t f = (size_t)b * a.T + t;
    const float* g = a.gamma + f * a.D;
    double e = 0.0;
    for (int k = 0; k < a.Kt; k++) {
      const int d = a.pdfs[f * a.Kt + k];
      if (d < 0) continue;
      if (d >= a.D) { bad++; continue; }
      e += (double)a.probs[f * a.Kt + k] * (double)g[d];
    }
    a.frame_acc[f] = (float)e;
    sum += e;
  }
  sum = wave_sum_f64(sum);
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((tid & 63) == 0) {
    red[tid >> 6] = sum;
    if (bad) atomicAdd(a.bad_count + 1, bad);                 // (an integer sum: the same value in any order)
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < kSmAccNT / 64; w++) s += red[w];
    a.acc_per_seq[b] = s;
  }
}

// The same by class: e(b,t) = sum_n gamma(b,t,n) Acls(t, cls[n]) is a dense pass over gamma, so a wave takes a frame on a grid over
// (frames, B) - kSmAccWaves frames a workgroup, no barrier.  The frame's entries are merged first: lane k keeps (class, summed q)
// of entry k where its class occurs first in the frame, q summed in ascending k (entries beyond 64: in chunks of a wave).  Every
// lane then walks its elements in ascending n against the merged entries, read lane by lane; the products are summed in fp64 per
// lane and over the wave by the butterfly.  E_b is summed from the fp64 frame values by a launch of its own.
constexpr int kSmAccWaves = kSmAccNT / 64;
template <int VW>
__global__ __launch_bounds__(kSmAccNT) void smbr_class_frame_acc_kernel(const SmbrAccArgs a, const SmbrClasses c) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int t = blockIdx.x * kSmAccWaves + (threadIdx.x >> 6);
  if (t >= seq_len(a.lengths, b, a.T)) return;                                 // (the whole wave)
  const size_t f = (size_t)b * a.T + t;
  const int32_t* pd = a.pdfs + f * a.Kt;
  const float* pr = a.probs + f * a.Kt;
  const float* g = a.gamma + f * a.D;
  const int D = a.D, Kt = a.Kt;
  double e = 0.0;
  int bad = 0;
  for (int k0 = 0; k0 < Kt; k0 += 64) {
    const int k = k0 + lane;
    int mc = -1;
    float mq = 0.f;
    if (k < Kt) {
      if (pd[k] >= (c.targets_are_classes ? c.C : D)) bad++;
      mc = entry_class(c, pd[k], D);
      for (int j = 0; j < k && mc >= 0; j++)
        if (entry_class(c, pd[j], D) == mc) mc = -1;
      if (mc >= 0) {
        mq = pr[k];
        for (int j = k + 1; j < Kt; j++)
          if (entry_class(c, pd[j], D) == mc) mq += pr[j];
      }
    }
    const int live = min(64, Kt - k0);
    for (int base = 0; base < D; base += 64 * VW) {                            // (the same trips in every lane: the lane reads below)
      const int n0 = base + lane * VW;
      float v[VW], av[VW];
      int cn[VW];
#pragma unroll
      for (int i = 0; i < VW; i++) { v[i] = 0.f; av[i] = 0.f; cn[i] = -2; }
      if (n0 < D) {
        row_load<kXF32, VW>(g, (size_t)n0, v);
        if constexpr (VW == 4) {
          const int4 q = *reinterpret_cast<const int4*>(c.cls + n0);
          cn[0] = q.x; cn[1] = q.y; cn[2] = q.z; cn[3] = q.w;
        } else {
          cn[0] = c.cls[n0];
        }
      }
      for (int j = 0; j < live; j++) {
        const int jc = __builtin_amdgcn_readlane(mc, j);
        const float jq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mq), j));
#pragma unroll
        for (int i = 0; i < VW; i++)
          if (cn[i] == jc) av[i] = jq;                                         // (at most one merged entry has the class)
      }
#pragma unroll
      for (int i = 0; i < VW; i++) e += (double)v[i] * (double)av[i];
    }
  }
  e = wave_sum_f64(e);
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if (lane == 0) {
    a.frame_acc[f] = (float)e;
    c.frame_e[f] = e;
    if (bad) atomicAdd(a.bad_count + 1, bad);                                  // (an integer sum: the same value in any order)
  }
}
// E_b = sum_t e(b,t) in fp64: one workgroup per sequence, a thread per frame, the order of smbr_frame_acc_kernel
__global__ __launch_bounds__(kSmAccNT) void smbr_class_seq_acc_kernel(const SmbrAccArgs a, const SmbrClasses c) {
  __shared__ double red[kSmAccNT / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int L = seq_len(a.lengths, b, a.T);
  double sum = 0.0;
  for (int t = tid; t < L; t += kSmAccNT) sum += c.frame_e[(size_t)b * a.T + t];
  sum = wave_sum_f64(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < kSmAccNT / 64; w++) s += red[w];
    a.acc_per_seq[b] = s;
  }
}

// ---- stage 2: the recursions ----------------------------------------------------------------------------------------------------
// (hold_row / put_row - row t of the sequence into LDS as exp(clamp(.)) -: smbr_device.h)
// x A of the elements put_row stored, by class: xacc[n] = xrow[n] * acl[cls[n]] - the thread reads back what it wrote itself;
// `hc`: cls of the elements held in registers, those beyond are loaded again
__device__ __forceinline__ void class_row(const int32_t* cls, const int (&hc)[kSmXR], int D, int tid, const float* acl, const float* xrow, float* xacc) {
#pragma unroll
  for (int i = 0; i < kSmXR; i++) {
    const int n = tid + i * kSmNT;
    if (n < D) xacc[n] = xrow[n] * acl[hc[i]];
  }
  for (int n = tid + kSmXR * kSmNT; n < D; n += kSmNT) xacc[n] = xrow[n] * acl[cls[n]];
}

// CLS: the accuracy by class (§3.27) - `c` is read, the table acl [C] lies behind the reduction scratch, and the companion row is
// dense: made from the next row and the next frame's table in the slot where the pdf-level form scatters its K entries.
template <int XH, bool FWD, bool CLS>
__device__ __forceinline__ void smbr_recursion(const SmbrArgs& a, const SmbrClasses& c, int b, float* lds) {
  const int tid = threadIdx.x;
  const SmbrGraph& g = a.g;
  const int H = g.H, D = a.D, T = a.T, Kt = a.Kt;
  const int L = seq_len(a.lengths, b, T);
  float* const vec0 = lds;                       // [2][H] alpha' / beta'
  float* const vec1 = lds + 2 * (size_t)H;       // [2][H] alpha-bar' / beta-bar'
  float* const xrow = vec1 + 2 * (size_t)H;      // [2][D] x
  float* const xacc = xrow + 2 * (size_t)D;      // [2][D] x * A
  float* const red = xacc + 2 * (size_t)D;
  float* const acl = red + kSmRed;               // [C] Acls of the frame whose companion row is made next (CLS)
  int hc[kSmXR];
  if constexpr (CLS) {
#pragma unroll
    for (int i = 0; i < kSmXR; i++) hc[i] = tid + i * kSmNT < D ? c.cls[tid + i * kSmNT] : 0;
  }
  const size_t seq_rows = (size_t)b * (T + 1);
  float* const st0 = (FWD ? a.al : a.be) + seq_rows * H;
  float* const st1 = (FWD ? a.ab : a.bb) + seq_rows * H;
  float* const totv = (FWD ? a.tot_a : a.tot_b) + seq_rows;
  const int32_t* const idx = FWD ? g.bi : g.fi;                // forwards: the arcs ENTERING a state; backwards: those leaving it
  const int32_t* const arc = FWD ? g.bt : g.ft;
  const float* const pr = FWD ? g.bp : g.fp;
  const float coef = a.coef;
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
      vec0[i] = v; vec1[i] = 0.f;
      st0[(size_t)r0 * H + i] = v; st1[(size_t)r0 * H + i] = 0.f;
    }
    const int t0 = FWD ? 0 : L - 1;
    float held[kSmXR];
    hold_row<XH>(a.x, xseq + (size_t)t0 * D, D, tid, held);
    nan = put_row<XH>(a.x, xseq + (size_t)t0 * D, D, tid, held, xrow) || nan;
    if constexpr (CLS) {
      class_table(c, a.pdfs + (fseq + t0) * Kt, a.probs + (fseq + t0) * Kt, Kt, D, tid, kSmNT, acl);
      __syncthreads();
      class_row(c.cls, hc, D, tid, acl, xrow, xacc);
    } else {
      for (int n = tid; n < D; n += kSmNT) xacc[n] = 0.f;
      __syncthreads();
      scatter_entries(a.pdfs + (fseq + t0) * Kt, a.probs + (fseq + t0) * Kt, Kt, D, tid, kSmNT, xrow, xacc);
    }
    __syncthreads();
  }
  // frame j: forwards alpha'(t+1) from alpha'(t) and x(t), t = j; backwards beta'(t) from beta'(t+1) and x(t), t = L-1-j
  for (int j = 0; j < L; j++) {
    const int p = j & 1;
    const int t = FWD ? j : L - 1 - j, tn = FWD ? t + 1 : t - 1;
    const bool more = j + 1 < L;
    const float* v0 = vec0 + (size_t)p * H;
    const float* v1 = vec1 + (size_t)p * H;
    float* w0 = vec0 + (size_t)(1 - p) * H;
    float* w1 = vec1 + (size_t)(1 - p) * H;
    const float* xr = xrow + (size_t)p * D;
    const float* xa = xacc + (size_t)p * D;
    float* xrn = xrow + (size_t)(1 - p) * D;
    float* xan = xacc + (size_t)(1 - p) * D;
    float held[kSmXR];
    if (more) hold_row<XH>(a.x, xseq + (size_t)tn * D, D, tid, held);          // the next frame's row: in flight over the arc loop
    if constexpr (CLS) {                                                       // (the table's readers are behind the last barrier)
      if (more) class_table(c, a.pdfs + (fseq + tn) * Kt, a.probs + (fseq + tn) * Kt, Kt, D, tid, kSmNT, acl);
    } else {
      for (int n = tid; n < D; n += kSmNT) xan[n] = 0.f;
    }
    const float e_t = a.frame_acc[fseq + t];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int i = tid; i < H; i += kSmNT) {
      float acc0 = 0.f, acc1 = 0.f;
      const int k1 = idx[2 * i + 1];
      for (int k = idx[2 * i]; k < k1; k++) {
        const int other = arc[3 * k + (FWD ? 0 : 1)], n = arc[3 * k + 2];
        const float w = pr[k], u0 = v0[other], u1 = v1[other], xx = xr[n], xq = xa[n];
        const float wu = w * u0;
        acc0 += wu * xx;
        acc1 += (w * u1) * xx + wu * xq;
      }
      acc1 -= e_t * acc0;                                                      // the centring: a(t,n) = A(t,n) - e(t)
      w0[i] = acc0; w1[i] = acc1;                                              // raw, finished below by the thread that wrote them
      s0 += acc0;
      if (FWD) s1 += acc1;
      else { s1 += acc0 * g.leaky[i]; s2 += acc1 * g.leaky[i]; }
    }
    if (more) nan = put_row<XH>(a.x, xseq + (size_t)tn * D, D, tid, held, xrn) || nan;
    block_sum3<kSmNT>(s0, s1, s2, red, tid);                                   // (its barrier: the next rows are whole)
    if constexpr (CLS) {
      if (more) class_row(c.cls, hc, D, tid, acl, xrn, xan);
    } else {
      if (more) scatter_entries(a.pdfs + (fseq + tn) * Kt, a.probs + (fseq + tn) * Kt, Kt, D, tid, kSmNT, xrn, xan);
    }
    const float inv = 1.f / s0;
    if (!(s0 > 0.f) || !(inv > 0.f) || !(inv - inv == 0.f)) bad = true;
    const int r = FWD ? t + 1 : t;
    if (tid == 0) totv[r] = s0;
    float* o0 = st0 + (size_t)r * H;
    float* o1 = st1 + (size_t)r * H;
    for (int i = tid; i < H; i += kSmNT) {
      float c0, c1;
      if (FWD) {
        const float lk = coef * g.leaky[i];
        c0 = w0[i] * inv + lk;                                                 // (the normalised alpha sums to one)
        c1 = (w1[i] + lk * s1) * inv;
      } else {
        c0 = (w0[i] + coef * s1) * inv;
        c1 = (w1[i] + coef * s2) * inv;
      }
      w0[i] = c0; w1[i] = c1;
      o0[i] = c0; o1[i] = c1;
    }
    __syncthreads();
  }
  // a NaN in a live row of x (the clamp turns it into exp(-30): watched here, by the forward workgroup), a total that is not
  // positive and finite: the sequence is bad.  (Both workgroups of a sequence may store the same 1.)
  if (__syncthreads_or((bad || (FWD && nan)) ? 1 : 0) && tid == 0) a.seq_bad[b] = 1;
}

template <int XH>
__global__ __launch_bounds__(kSmNT) void smbr_recursion_kernel(const SmbrArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  if (blockIdx.x < (unsigned)a.B) smbr_recursion<XH, true, false>(a, SmbrClasses{}, blockIdx.x, lds);
  else smbr_recursion<XH, false, false>(a, SmbrClasses{}, blockIdx.x - a.B, lds);
}
template <int XH>
__global__ __launch_bounds__(kSmNT) void smbr_class_recursion_kernel(const SmbrArgs a, const SmbrClasses c) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  if (blockIdx.x < (unsigned)a.B) smbr_recursion<XH, true, true>(a, c, blockIdx.x, lds);
  else smbr_recursion<XH, false, true>(a, c, blockIdx.x - a.B, lds);
}

// ---- stage 2: the gradient ------------------------------------------------------------------------------------------------------
// (smbr_condemn - a sequence that went bad is counted once, its E_b NaN -: smbr_device.h)
template <int XH>
__global__ __launch_bounds__(kSmGNT) void smbr_grad_kernel(const SmbrArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  const int tid = threadIdx.x, b = blockIdx.y;
  const SmbrGraph& g = a.g;
  const int H = g.H, D = a.D, T = a.T, Kt = a.Kt;
  const int L = seq_len(a.lengths, b, T);
  float* const sa = lds;                          // alpha'(t)
  float* const sab = sa + H;                      // alpha-bar'(t)
  float* const sb = sab + H;                      // beta'(t+1)
  float* const sbb = sb + H;                      // beta-bar'(t+1)
  float* const gq = sbb + H;                      // [D] x q0
  float* const gv = gq + D;                       // [D] x (q1 - e q0), then + A x q0 where the frame has an entry
  float* const red = gv + D;
  const size_t seq_rows = (size_t)b * (T + 1);
  const float gscale = a.grad_scale_dev ? a.grad_scale * *a.grad_scale_dev : a.grad_scale;
  const int t_begin = blockIdx.x * kSmFrames, t_end = min(t_begin + kSmFrames, T);
  for (int t = t_begin; t < t_end; t++) {
    const size_t row = ((size_t)b * T + t) * D;
    if (t >= L) {                                                              // padding: exact zeros
      for (int n = tid; n < D; n += kSmGNT) row_store1<XH>(a.grad, row + n, 0.f);
      continue;
    }
    const size_t r0 = (seq_rows + t) * H, r1 = r0 + H;
    for (int i = tid; i < H; i += kSmGNT) { sa[i] = a.al[r0 + i]; sab[i] = a.ab[r0 + i]; sb[i] = a.be[r1 + i]; sbb[i] = a.bb[r1 + i]; }
    __syncthreads();
    const float e_t = a.frame_acc[(size_t)b * T + t];
    float part = 0.f, none1 = 0.f, none2 = 0.f;
    for (int n = tid; n < D; n += kSmGNT) {
      const int k0 = g.pidx[n], k1 = g.pidx[n + 1];
      float q0 = 0.f, q1 = 0.f;
      for (int k = k0; k < k1; k++) {
        const int id = g.parc[k];
        const int src = g.ft[3 * id], dst = g.ft[3 * id + 1];
        const float w = g.fp[id];
        const float wa = w * sa[src];
        q0 += wa * sb[dst];
        q1 += (w * sab[src]) * sb[dst] + wa * sbb[dst];
      }
      float v0 = 0.f, v1 = 0.f;
      if (k0 != k1) {                                                          // a pdf no arc carries: its x is not read
        const float xx = clamp_exp(row_load1<XH>(a.x, row + n), kXExpClamp);
        v0 = xx * q0;
        v1 = xx * (q1 - e_t * q0);
      }
      gq[n] = v0; gv[n] = v1;
      part += v0;
    }
    block_sum3<kSmGNT>(part, none1, none2, red, tid);
    {
      const int32_t* pd = a.pdfs + ((size_t)b * T + t) * Kt;
      const float* pr = a.probs + ((size_t)b * T + t) * Kt;
      int d;
      float q;
      for (int k = tid; k < Kt; k += kSmGNT)
        if (owned_entry(pd, pr, k, Kt, D, d, q)) gv[d] += q * gq[d];
    }
    __syncthreads();
    // The row's mean: a second sum, over the FINISHED elements.  (Summing x (q1 - e q0) in the first block sum and the owners'
    // A x q0 beside it gives the same mean in exact arithmetic, but at a pdf with gamma near one the two halves are each as large
    // as the divisor and cancel: the mean must carry the rounding its elements carry, or it spreads 1e-7 of gamma over the row.)
    // Its scratch is red[48 ..], which block_sum3 leaves alone - slower waves may still read red[0 .. 47].
    float mean = 0.f;
    for (int n = tid; n < D; n += kSmGNT) mean += gv[n];
    mean = wave_sum(mean);
    if ((tid & 63) == 0) red[48 + (tid >> 6)] = mean;
    __syncthreads();
    mean = 0.f;
    for (int w = 0; w < kSmGNT / 64; w++) mean += red[48 + w];                   // (same order in every thread)
    const float sc = gscale / part, inv = 1.f / part;
    if ((!(part > 0.f) || !(inv - inv == 0.f)) && tid == 0) smbr_condemn(a, b);    // (the host twin's check of the same divisor)
    // The row is centred by its own mean, as smbr_class_grad_kernel's: sum_n x (q1 + a q0) is zero but for the rounding of e(t),
    // and that residue enters alpha-bar and beta-bar at every frame and stays - uncentred, the row carries gamma(t,n) times the
    // residue accumulated over the sequence (`closing` is that sum; DESIGN.md §3.26, "The residue").
    const float eps = mean * inv;
    for (int n = tid; n < D; n += kSmGNT) {
      const bool carried = g.pidx[n] != g.pidx[n + 1];
      row_store1<XH>(a.grad, row + n, carried ? (gv[n] - eps * gq[n]) * sc : 0.f);
    }
    __syncthreads();                                                           // (the rows are free for the next frame)
  }
  // the sequence's first workgroup closes it: the diagnostic sum_j alpha-bar'(L,j) final(j) / sum_j alpha'(L,j) final(j), and the
  // sequence's verdict
  if (blockIdx.x == 0) {
    const size_t rL = (seq_rows + L) * H;
    float c0 = 0.f, c1 = 0.f, none = 0.f;
    for (int i = tid; i < H; i += kSmGNT) { c0 += a.al[rL + i] * g.fin[i]; c1 += a.ab[rL + i] * g.fin[i]; }
    block_sum3<kSmGNT>(c0, c1, none, red, tid);
    if (tid == 0) {
      const bool bad = a.seq_bad[b] != 0 || !(c0 > 0.f);                       // what the recursions found
      a.closing[b] = bad ? __builtin_nanf("") : c1 / c0;
      if (bad) smbr_condemn(a, b);
    }
  }
}

// The same by class (§3.27): smbr_grad_kernel with the frame's table acl [C] made beside the state rows, and every carried pdf
// taking its class's credit in the pass that forms it, where the pdf-level form adds the K owned entries behind the reduction.
template <int XH>
__global__ __launch_bounds__(kSmGNT) void smbr_class_grad_kernel(const SmbrArgs a, const SmbrClasses c) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  const int tid = threadIdx.x, b = blockIdx.y;
  const SmbrGraph& g = a.g;
  const int H = g.H, D = a.D, T = a.T, Kt = a.Kt;
  const int L = seq_len(a.lengths, b, T);
  float* const sa = lds;                          // alpha'(t)
  float* const sab = sa + H;                      // alpha-bar'(t)
  float* const sb = sab + H;                      // beta'(t+1)
  float* const sbb = sb + H;                      // beta-bar'(t+1)
  float* const gq = sbb + H;                      // [D] x q0
  float* const gv = gq + D;                       // [D] x (q1 + a q0)
  float* const red = gv + D;
  float* const acl = red + kSmRed;                // [C] Acls of the frame
  const size_t seq_rows = (size_t)b * (T + 1);
  const float gscale = a.grad_scale_dev ? a.grad_scale * *a.grad_scale_dev : a.grad_scale;
  const int t_begin = blockIdx.x * kSmFrames, t_end = min(t_begin + kSmFrames, T);
  for (int t = t_begin; t < t_end; t++) {
    const size_t row = ((size_t)b * T + t) * D;
    if (t >= L) {                                                              // padding: exact zeros
      for (int n = tid; n < D; n += kSmGNT) row_store1<XH>(a.grad, row + n, 0.f);
      continue;
    }
    const size_t r0 = (seq_rows + t) * H, r1 = r0 + H;
    for (int i = tid; i < H; i += kSmGNT) { sa[i] = a.al[r0 + i]; sab[i] = a.ab[r0 + i]; sb[i] = a.be[r1 + i]; sbb[i] = a.bb[r1 + i]; }
    class_table(c, a.pdfs + ((size_t)b * T + t) * Kt, a.probs + ((size_t)b * T + t) * Kt, Kt, D, tid, kSmGNT, acl);
    __syncthreads();
    const float e_t = a.frame_acc[(size_t)b * T + t];
    float part = 0.f, none1 = 0.f, none2 = 0.f;
    for (int n = tid; n < D; n += kSmGNT) {
      const int k0 = g.pidx[n], k1 = g.pidx[n + 1];
      float q0 = 0.f, q1 = 0.f;
      for (int k = k0; k < k1; k++) {
        const int id = g.parc[k];
        const int src = g.ft[3 * id], dst = g.ft[3 * id + 1];
        const float w = g.fp[id];
        const float wa = w * sa[src];
        q0 += wa * sb[dst];
        q1 += (w * sab[src]) * sb[dst] + wa * sbb[dst];
      }
      float v0 = 0.f, v1 = 0.f;
      if (k0 != k1) {                                                          // a pdf no arc carries: its x is not read
        const float xx = clamp_exp(row_load1<XH>(a.x, row + n), kXExpClamp);
        v0 = xx * q0;
        v1 = xx * (q1 - e_t * q0);
        v1 += acl[c.cls[n]] * v0;                                             // (+ A x q0: the thread's own element)
      }
      gq[n] = v0; gv[n] = v1;
      part += v0;
      none1 += v1;
    }
    block_sum3<kSmGNT>(part, none1, none2, red, tid);                          // (below a thread reads its own elements only)
    const float sc = gscale / part, inv = 1.f / part;
    if ((!(part > 0.f) || !(inv - inv == 0.f)) && tid == 0) smbr_condemn(a, b);    // (the host twin's check of the same divisor)
    // The row is centred by its own mean: sum_n x (q1 + a q0) is zero but for the rounding of e(t) - the occupancies are another
    // kernel's, in fp32 -, and with a dense A of order one that residue, times gamma(t,n), is what the row would carry.
    const float eps = none1 * inv;
    for (int n = tid; n < D; n += kSmGNT) {
      const bool carried = g.pidx[n] != g.pidx[n + 1];
      row_store1<XH>(a.grad, row + n, carried ? (gv[n] - eps * gq[n]) * sc : 0.f);
    }
    __syncthreads();                                                           // (the rows are free for the next frame)
  }
  // the sequence's first workgroup closes it: the diagnostic sum_j alpha-bar'(L,j) final(j) / sum_j alpha'(L,j) final(j), and the
  // sequence's verdict
  if (blockIdx.x == 0) {
    const size_t rL = (seq_rows + L) * H;
    float c0 = 0.f, c1 = 0.f, none = 0.f;
    for (int i = tid; i < H; i += kSmGNT) { c0 += a.al[rL + i] * g.fin[i]; c1 += a.ab[rL + i] * g.fin[i]; }
    block_sum3<kSmGNT>(c0, c1, none, red, tid);
    if (tid == 0) {
      const bool bad = a.seq_bad[b] != 0 || !(c0 > 0.f);                       // what the recursions found
      a.closing[b] = bad ? __builtin_nanf("") : c1 / c0;
      if (bad) smbr_condemn(a, b);
    }
  }
}
template <int XH>
hipError_t launch_classes_as(const SmbrArgs& a, const SmbrClasses& c, hipStream_t st) {
  const size_t lds_r = smbr_recursion_lds(a.g.H, a.D, c.C), lds_g = smbr_grad_lds(a.g.H, a.D, c.C);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(smbr_class_recursion_kernel<XH>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(smbr_class_grad_kernel<XH>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((smbr_class_recursion_kernel<XH>), dim3(2 * a.B), dim3(kSmNT), lds_r, st, a, c);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((smbr_class_grad_kernel<XH>), dim3((a.T + kSmFrames - 1) / kSmFrames, a.B), dim3(kSmGNT), lds_g, st, a, c);
  return hipGetLastError();
}

template <int XH>
hipError_t launch_as(const SmbrArgs& a, hipStream_t st) {
  const size_t lds_r = smbr_recursion_lds(a.g.H, a.D), lds_g = smbr_grad_lds(a.g.H, a.D);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(smbr_recursion_kernel<XH>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(smbr_grad_kernel<XH>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((smbr_recursion_kernel<XH>), dim3(2 * a.B), dim3(kSmNT), lds_r, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((smbr_grad_kernel<XH>), dim3((a.T + kSmFrames - 1) / kSmFrames, a.B), dim3(kSmGNT), lds_g, st, a);
  return hipGetLastError();
}

}  // namespace

size_t smbr_recursion_lds(int H, int D) { return (4 * (size_t)H + 4 * (size_t)D + kSmRed) * sizeof(float); }
size_t smbr_grad_lds(int H, int D) { return (4 * (size_t)H + 2 * (size_t)D + kSmRed) * sizeof(float); }
size_t smbr_recursion_lds(int H, int D, int C) { return smbr_recursion_lds(H, D) + (size_t)C * sizeof(float); }
size_t smbr_grad_lds(int H, int D, int C) { return smbr_grad_lds(H, D) + (size_t)C * sizeof(float); }
size_t smbr_lds_bytes(int H, int D, int C) {       // (the gradient kernel has no static LDS, and fewer rows)
  const size_t r = smbr_recursion_lds(H, D, C) + kSmStaticLds, g = smbr_grad_lds(H, D, C);
  return r > g ? r : g;
}

hipError_t launch_smbr_frame_acc(const SmbrAccArgs& a, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.bad_count, 0, 2 * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(smbr_frame_acc_kernel, dim3(a.B), dim3(kSmAccNT), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_smbr(const SmbrArgs& a, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.seq_bad, 0, 2 * (size_t)a.B * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  if (a.x_half == kXF32) return launch_as<kXF32>(a, st);
  if (a.x_half == kXBf16) return launch_as<kXBf16>(a, st);
  return launch_as<kXF16>(a, st);
}

hipError_t launch_smbr_frame_acc(const SmbrAccArgs& a, const SmbrClasses& c, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.bad_count, 0, 2 * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  const dim3 grid((a.T + kSmAccWaves - 1) / kSmAccWaves, a.B);
  // float4 / int4 loads where every row of gamma and the map start on the 16-byte grid, else one element at a time
  const bool wide = a.D % 4 == 0 && ((uintptr_t)a.gamma | (uintptr_t)c.cls) % 16 == 0;
  if (wide) hipLaunchKernelGGL(smbr_class_frame_acc_kernel<4>, grid, dim3(kSmAccNT), 0, st, a, c);
  else hipLaunchKernelGGL(smbr_class_frame_acc_kernel<1>, grid, dim3(kSmAccNT), 0, st, a, c);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(smbr_class_seq_acc_kernel, dim3(a.B), dim3(kSmAccNT), 0, st, a, c);
  return hipGetLastError();
}

hipError_t launch_smbr(const SmbrArgs& a, const SmbrClasses& c, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.seq_bad, 0, 2 * (size_t)a.B * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  if (a.x_half == kXF32) return launch_classes_as<kXF32>(a, c, st);
  if (a.x_half == kXBf16) return launch_classes_as<kXBf16>(a, c, st);
  return launch_classes_as<kXF16>(a, c, st);
}

}  // namespace pychain_hip

using namespace pychain_hip;

// ---- the entry points (include/pychain_hip.h) -----------------------------------------------------------------------------------
namespace {
struct SmbrCarve { size_t al, ab, be, bb, tot_a, tot_b, seq_bad, end, total; };
SmbrCarve smbr_carve(int B, int T, int H) {
  SmbrCarve c;
  const size_t traj = align256((size_t)B * (T + 1) * H * sizeof(float)), tot = align256((size_t)B * (T + 1) * sizeof(float));
  size_t o = 0;
  c.al = o; o += traj; c.ab = o; o += traj; c.be = o; o += traj; c.bb = o; o += traj;
  c.tot_a = o; o += tot; c.tot_b = o; o += tot;
  c.seq_bad = o; o += align256(2 * (size_t)B * sizeof(int32_t));
  c.end = o;
  c.total = o + 256;                               // (the base is aligned inside the caller's buffer)
  return c;
}
// the general kernels' scratch rows (smbr.h: SmbrGeneral) behind the layout above, which they keep
struct SmbrGeneralCarve { size_t rec, grad, total; SmbrGeneral s; };
SmbrGeneralCarve smbr_general_carve(const SmbrCarve& c, int B, int T, int D, int C) {
  SmbrGeneralCarve v;
  memset(&v, 0, sizeof(v));
  v.s.rec_stride = smbr_general_rec_stride(D, C);
  v.s.grad_stride = smbr_general_grad_stride(D, C);
  v.s.grad_wgs = smbr_general_grad_wgs(B, T);
  size_t o = c.end;
  v.rec = o; o += align256(2 * (size_t)B * v.s.rec_stride * sizeof(float));
  v.grad = o; o += align256((size_t)v.s.grad_wgs * v.s.grad_stride * sizeof(float));
  v.total = o + 256;
  return v;
}

// The form a call of the general entry point runs (include/pychain_hip.h: PYCHAIN_HIP_SMBR_*), or a negative code with the
// message set.  C = 0: the pdf-level call.
int smbr_resolve_form(const char* who, int H, int D, int C, int requested) {
  if (H <= 0 || D <= 0 || C < 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes H=%d D=%d num_classes=%d", who, H, D, C);
  if (requested < PYCHAIN_HIP_SMBR_AUTO || requested > PYCHAIN_HIP_SMBR_GLOBAL)
    return fail(PYCHAIN_HIP_EINVAL, "%s: unknown form %d (PYCHAIN_HIP_SMBR_AUTO .. _GLOBAL)", who, requested);
  const size_t lds = smbr_lds_bytes(H, D, C), rows = smbr_general_lds(H);
  if (requested == PYCHAIN_HIP_SMBR_LDS && lds > kSmbrLdsBudget)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: the LDS form needs %zu bytes of LDS for %d states, %d pdfs and %d classes (four state vectors, four rows and the class table), a CU has %zu",
                who, lds, H, D, C, kSmbrLdsBudget);
  if (requested == PYCHAIN_HIP_SMBR_ROWS && rows > kSmbrLdsBudget)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: the rows form needs %zu bytes of LDS for %d states (four state vectors), a CU has %zu",
                who, rows, H, kSmbrLdsBudget);
  if (requested != PYCHAIN_HIP_SMBR_AUTO) return requested;
  return lds <= kSmbrLdsBudget ? PYCHAIN_HIP_SMBR_LDS : rows <= kSmbrLdsBudget ? PYCHAIN_HIP_SMBR_ROWS : PYCHAIN_HIP_SMBR_GLOBAL;
}
constexpr int kSmbrFormOfOld = -1;                 // the two entry points from before the general kernels: LDS or refused, their messages
}  // namespace

extern "C" int pychain_hip_smbr_form(int H, int D, int num_classes, int requested) {
  return smbr_resolve_form("smbr_form", H, D, num_classes, requested);
}

extern "C" size_t pychain_hip_smbr_general_lds_bytes(int H) {
  if (H <= 0) return 0;
  return smbr_general_lds(H);
}

extern "C" size_t pychain_hip_smbr_general_workspace_bytes(int B, int T, int H, int D, int num_classes) {
  if (B <= 0 || T <= 0 || H <= 0 || D <= 0 || num_classes < 0) return 0;
  return smbr_general_carve(smbr_carve(B, T, H), B, T, D, num_classes).total;
}

extern "C" size_t pychain_hip_smbr_workspace_bytes(int B, int T, int H) {
  if (B <= 0 || T <= 0 || H <= 0) return 0;
  return smbr_carve(B, T, H).total;
}

extern "C" size_t pychain_hip_smbr_frame_accuracy_classes_workspace_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  return align256((size_t)B * T * sizeof(double)) + 256;
}

extern "C" size_t pychain_hip_smbr_lds_bytes(int H, int D, int num_classes) {
  if (H <= 0 || D <= 0 || num_classes < 0) return 0;
  return smbr_lds_bytes(H, D, num_classes);
}

namespace {
// what a class call says of its map: `cls` is the caller's, non-null
int bad_classes(const char* who, int num_classes) {
  if (num_classes < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: num_classes must be at least 1 with pdf_classes, got %d", who, num_classes);
  return PYCHAIN_HIP_OK;
}
int classes_without_map(const char* who) {
  return fail(PYCHAIN_HIP_EINVAL, "%s: targets_are_classes needs pdf_classes", who);
}

// both accuracy entry points; `pdf_classes` null: the pdf-level launch
int smbr_frame_accuracy(const char* who, const float* gamma, const int64_t* seq_lengths, int B, int T, int D,
                        const int32_t* target_pdfs, const float* target_probs, int K,
                        float* frame_acc, double* acc_per_seq, int32_t* bad_count, void* stream,
                        const int32_t* pdf_classes, int num_classes, int targets_are_classes, void* workspace, size_t workspace_bytes) {
  if (!gamma || !seq_lengths || !target_pdfs || !target_probs || !frame_acc || !acc_per_seq || !bad_count) return null_pointer(who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  if ((size_t)B * T > (size_t)INT_MAX) return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: B * T = %zu frames", who, (size_t)B * T);
  SmbrAccArgs a;
  memset(&a, 0, sizeof(a));
  a.gamma = gamma; a.lengths = seq_lengths; a.pdfs = target_pdfs; a.probs = target_probs; a.frame_acc = frame_acc;
  a.acc_per_seq = acc_per_seq; a.bad_count = bad_count; a.B = B; a.T = T; a.D = D; a.Kt = K;
  hipError_t err;
  if (pdf_classes) {
    const int rc = bad_classes(who, num_classes);
    if (rc != PYCHAIN_HIP_OK) return rc;
    if (!workspace) return null_pointer(who);
    const size_t need = pychain_hip_smbr_frame_accuracy_classes_workspace_bytes(B, T);
    if (workspace_bytes < need) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    const SmbrClasses c{pdf_classes, num_classes, targets_are_classes != 0, (double*)ws_base(workspace)};
    err = launch_smbr_frame_acc(a, c, (hipStream_t)stream);
  } else {
    err = launch_smbr_frame_acc(a, (hipStream_t)stream);
  }
  if (err != hipSuccess) return launch_failed(who, err, nullptr);
  return PYCHAIN_HIP_OK;
}
}  // namespace

extern "C" int pychain_hip_smbr_frame_accuracy(const float* gamma, const int64_t* seq_lengths, int B, int T, int D,
                                               const int32_t* target_pdfs, const float* target_probs, int K,
                                               float* frame_acc, double* acc_per_seq, int32_t* bad_count, void* stream) {
  return smbr_frame_accuracy("smbr_frame_accuracy", gamma, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc, acc_per_seq, bad_count,
                             stream, nullptr, 0, 0, nullptr, 0);
}

extern "C" int pychain_hip_smbr_frame_accuracy_classes(const float* gamma, const int64_t* seq_lengths, int B, int T, int D,
                                                       const int32_t* target_pdfs, const float* target_probs, int K,
                                                       float* frame_acc, double* acc_per_seq, int32_t* bad_count, void* stream,
                                                       const int32_t* pdf_classes, int num_classes, int targets_are_classes,
                                                       void* workspace, size_t workspace_bytes) {
  if (!pdf_classes) {                              // the pdf-level call, launch for launch
    if (targets_are_classes) return classes_without_map("smbr_frame_accuracy_classes");
    return pychain_hip_smbr_frame_accuracy(gamma, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc, acc_per_seq, bad_count, stream);
  }
  return smbr_frame_accuracy("smbr_frame_accuracy_classes", gamma, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc, acc_per_seq,
                             bad_count, stream, pdf_classes, num_classes, targets_are_classes, workspace, workspace_bytes);
}

namespace {
// both recursion entry points; `pdf_classes` null: the pdf-level launches
int smbr_forward_backward(
    const char* who,
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes, int form) {
  const NumGraphs graphs{ft, fi, fp, bt, bi, bp, initial, final_, 0, H, num_arcs};
  const Rows rows{nnet_output, nnet_output_dtype, seq_lengths, B, T, D};
  int rc = bad_dtype(who, nnet_output_dtype);
  if (rc != PYCHAIN_HIP_OK) return rc;
  if (graphs.any_null() || !leaky || !pdf_arcs || !pdf_index || !rows.x || !rows.lengths || !target_pdfs || !target_probs || !frame_acc ||
      !grad || !acc_per_seq || !closing || !bad_count || !workspace)
    return null_pointer(who);
  if ((rc = bad_sizes(who, rows, graphs)) != PYCHAIN_HIP_OK) return rc;
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  if (!(leaky_hmm_coefficient > 0.f && leaky_hmm_coefficient < 1.f))
    return fail(PYCHAIN_HIP_EINVAL, "%s: leaky_hmm_coefficient must be in (0,1), got %g", who, (double)leaky_hmm_coefficient);
  if (pdf_classes && (rc = bad_classes(who, num_classes)) != PYCHAIN_HIP_OK) return rc;
  const int C = pdf_classes ? num_classes : 0;
  int run = PYCHAIN_HIP_SMBR_LDS;
  if (form == kSmbrFormOfOld) {
    if (pdf_classes) {
      const size_t need = smbr_lds_bytes(H, D, num_classes);
      if (need > kSmbrLdsBudget)
        return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: %d states, %d pdfs and %d classes need %zu bytes of LDS (four state vectors, four rows and the class table), a CU has %zu",
                    who, H, D, num_classes, need, kSmbrLdsBudget);
    }
    const size_t lds = smbr_recursion_lds(H, D);
    if (!pdf_classes && lds + kSmStaticLds > kSmbrLdsBudget)
      return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: %d states and %d pdfs need %zu bytes of LDS (four state vectors and four rows), a CU has %zu",
                  who, H, D, lds + kSmStaticLds, kSmbrLdsBudget);
  } else if ((run = smbr_resolve_form(who, H, D, C, form)) < 0) {
    return run;
  }
  if ((size_t)B * (T + 1) > (size_t)INT_MAX) return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: B * (T + 1) = %zu rows", who, (size_t)B * (T + 1));
  const SmbrCarve c = smbr_carve(B, T, H);
  SmbrGeneralCarve gc = smbr_general_carve(c, B, T, D, C);
  const size_t ws_need = run == PYCHAIN_HIP_SMBR_LDS ? c.total : gc.total;     // (the LDS form takes the trajectories alone)
  if (workspace_bytes < ws_need) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, ws_need);
  char* base = ws_base(workspace);
  SmbrArgs a;
  memset(&a, 0, sizeof(a));
  a.g = SmbrGraph{ft, fi, fp, bt, bi, bp, leaky, initial, final_, pdf_arcs, pdf_index, H, num_arcs};
  a.x = nnet_output; a.x_half = nnet_output_dtype; a.lengths = seq_lengths; a.pdfs = target_pdfs; a.probs = target_probs;
  a.frame_acc = frame_acc; a.coef = leaky_hmm_coefficient; a.grad_scale = grad_scale; a.grad_scale_dev = grad_scale_dev;
  a.grad = grad; a.acc_per_seq = acc_per_seq; a.closing = closing; a.bad_count = bad_count;
  a.al = (float*)(base + c.al); a.ab = (float*)(base + c.ab); a.be = (float*)(base + c.be); a.bb = (float*)(base + c.bb);
  a.tot_a = (float*)(base + c.tot_a); a.tot_b = (float*)(base + c.tot_b); a.seq_bad = (int32_t*)(base + c.seq_bad);
  a.B = B; a.T = T; a.D = D; a.Kt = K;
  const SmbrClasses cl{pdf_classes, C, targets_are_classes != 0, nullptr};
  hipError_t err;
  if (run == PYCHAIN_HIP_SMBR_LDS) {
    err = pdf_classes ? launch_smbr(a, cl, (hipStream_t)stream) : launch_smbr(a, (hipStream_t)stream);
  } else {
    gc.s.rec = (float*)(base + gc.rec); gc.s.grad = (float*)(base + gc.grad);
    gc.s.state_lds = run == PYCHAIN_HIP_SMBR_ROWS;
    err = launch_smbr_general(a, cl, gc.s, (hipStream_t)stream);
  }
  if (err != hipSuccess) return launch_failed(who, err, nullptr);
  return PYCHAIN_HIP_OK;
}
}  // namespace

extern "C" int pychain_hip_smbr_forward_backward(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream) {
  return smbr_forward_backward("smbr_forward_backward", ft, fi, fp, bt, bi, bp, leaky, initial, final_, pdf_arcs, pdf_index, H, num_arcs,
                               nnet_output, nnet_output_dtype, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc,
                               leaky_hmm_coefficient, grad_scale, grad_scale_dev, grad, acc_per_seq, closing, bad_count,
                               workspace, workspace_bytes, stream, nullptr, 0, 0, kSmbrFormOfOld);
}

extern "C" int pychain_hip_smbr_forward_backward_classes(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes) {
  if (!pdf_classes && targets_are_classes) return classes_without_map("smbr_forward_backward_classes");
  return smbr_forward_backward(pdf_classes ? "smbr_forward_backward_classes" : "smbr_forward_backward", ft, fi, fp, bt, bi, bp, leaky, initial,
                               final_, pdf_arcs, pdf_index, H, num_arcs, nnet_output, nnet_output_dtype, seq_lengths, B, T, D, target_pdfs,
                               target_probs, K, frame_acc, leaky_hmm_coefficient, grad_scale, grad_scale_dev, grad, acc_per_seq, closing,
                               bad_count, workspace, workspace_bytes, stream, pdf_classes, num_classes, targets_are_classes, kSmbrFormOfOld);
}

// any H, num_pdfs, num_classes: `form` picks the kernels, PYCHAIN_HIP_SMBR_LDS today's launches
extern "C" int pychain_hip_smbr_forward_backward_general(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes, int form) {
  if (!pdf_classes && targets_are_classes) return classes_without_map("smbr_forward_backward_general");
  if (form < PYCHAIN_HIP_SMBR_AUTO || form > PYCHAIN_HIP_SMBR_GLOBAL)
    return fail(PYCHAIN_HIP_EINVAL, "smbr_forward_backward_general: unknown form %d (PYCHAIN_HIP_SMBR_AUTO .. _GLOBAL)", form);
  return smbr_forward_backward("smbr_forward_backward_general", ft, fi, fp, bt, bi, bp, leaky, initial, final_, pdf_arcs, pdf_index, H, num_arcs,
                               nnet_output, nnet_output_dtype, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc,
                               leaky_hmm_coefficient, grad_scale, grad_scale_dev, grad, acc_per_seq, closing, bad_count,
                               workspace, workspace_bytes, stream, pdf_classes, num_classes, targets_are_classes, form);
}
