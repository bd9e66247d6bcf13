// smbr_general.hip - lattice-free sMBR for graphs and trees the LDS kernels of smbr.hip do not take (DESIGN.md §3.28;
// include/pychain_hip.h: pychain_hip_smbr_forward_backward_general): four state vectors and four rows of a frame beyond the 160 KiB
// of a CU - 3000 states with more than about 7 200 pdfs, identity classes sooner, more than about 10 000 states at any D.  As
// den_general.hip is to the compiled-plan kernels: SLOW - what does not fit LDS is gathered from global memory, L2-resident at
// best - but complete, any H, K, D, C that the int32 reference layout holds, with the decomposition, the workspace layout and the
// checks of smbr.hip, so everything around the two launches is shared.
//
//   smbr_general_recursion_kernel<XH, CLS, VLDS>   2B persistent workgroups of 1024, one per (sequence, direction); a thread owns
//                                  states tid, tid + 1024, ..., arcs in the reference layout: smbr_recursion, statement by statement.
//                                  The frame's row x = exp(clamp(y)), its companion x A and the class table lie in scratch rows of
//                                  the workspace, the two rows double-buffered and made a frame ahead, as the LDS kernel makes them.
//                                  VLDS ("rows"): both state vectors double-buffered in LDS, 4 H floats.  !VLDS ("global"): the
//                                  previous state rows are read back from the trajectory store the workgroup has just written.
//   smbr_general_grad_kernel<XH, CLS>   at most kSmbrGradMaxWgs workgroups of 512, persistent over the (sequence, block of 8 frames)
//                                  items; a thread owns pdfs tid, tid + 512, ...; the four state rows are gathered straight from
//                                  the trajectories (written by the launch before: plain loads), the two D-rows x q0 and
//                                  x (q1 + a q0) and the class table lie in scratch rows of the workgroup.
//
// Staged rows, not a gather of y per arc: C4's graph has 30 000 arcs on 8408 pdfs, so a gather exp's every element 3.6 times a
// frame and direction on the arc loop's dependent chain, and it would need the frame's K target entries searched per arc (or the
// class table read through a second dependent gather).  The forward workgroup has to pass over all D elements of a live row in any
// case - a NaN on a pdf no arc carries is a NaN loss -, and that pass stages the row for one store more an element.
//
// A value another thread of the workgroup wrote to global memory before the last barrier is read as den_general.hip reads it:
// load_fresh (around the vector L1, which other waves' stores do not refresh) behind `__threadfence(); __syncthreads();`.
//
// SAME BITS.  Thread-to-state and thread-to-pdf ownership, the arc order and the order of every sum are those of smbr.hip (the
// shared code is one copy: smbr_device.h), and this unit too is compiled with contraction off: where both run, the general kernels
// give the bits of the LDS kernels (tests/test_gpu_smbr_general.py).  Nothing is atomic but integer counters and flags.
#include <hip/hip_runtime.h>

#include <cstring>

#pragma clang fp contract(off)      // ahead of the project's headers: their inline helpers (clamp_exp, the row loads) are under it too

#include "../../include/pychain_hip.h"
#include "common.h"
#include "row_access.h"
#include "smbr.h"
#include "smbr_device.h"

namespace pychain_hip {
namespace {

// a float written by another thread of this workgroup before the last barrier: read around the (non-coherent) vector L1
__device__ __forceinline__ float load_fresh(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// smbr.hip's class_row over scratch rows: xacc[n] = xrow[n] * acl[cls[n]] for the elements put_row stored
__device__ __forceinline__ void class_row_general(const int32_t* cls, const int (&hc)[kSmXR], int D, int tid, const float* acl, const float* xrow, float* xacc) {
#pragma unroll
  for (int i = 0; i < kSmXR; i++) {
    const int n = tid + i * kSmNT;
    if (n < D) xacc[n] = load_fresh(xrow + n) * load_fresh(acl + hc[i]);
  }
  for (int n = tid + kSmXR * kSmNT; n < D; n += kSmNT) xacc[n] = load_fresh(xrow + n) * load_fresh(acl + cls[n]);
}

// smbr.hip's smbr_recursion with `scratch` (x [2][D], x A [2][D], Acls [C]) in global memory; lds: red [kSmRed], then with VLDS
// the state vectors [2][H], [2][H]
template <int XH, bool FWD, bool CLS, bool VLDS>
__device__ __forceinline__ void smbr_general_recursion(const SmbrArgs& a, const SmbrClasses& c, float* scratch, int b, float* lds) {
  const int tid = threadIdx.x;
  const SmbrGraph& g = a.g;
  const int H = g.H, D = a.D, T = a.T, Kt = a.Kt;
  const int L = seq_len(a.lengths, b, T);
  float* const red = lds;
  float* const vec0 = lds + kSmRed;              // [2][H] alpha' / beta' (VLDS)
  float* const vec1 = vec0 + 2 * (size_t)H;      // [2][H] alpha-bar' / beta-bar' (VLDS)
  float* const xrow = scratch;                   // [2][D] x
  float* const xacc = xrow + 2 * (size_t)D;      // [2][D] x * A
  float* const acl = xacc + 2 * (size_t)D;       // [C] Acls of the frame whose companion row is made next (CLS)
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
      if constexpr (VLDS) { vec0[i] = v; vec1[i] = 0.f; }
      st0[(size_t)r0 * H + i] = v; st1[(size_t)r0 * H + i] = 0.f;
    }
    const int t0 = FWD ? 0 : L - 1;
    float held[kSmXR];
    hold_row<XH>(a.x, xseq + (size_t)t0 * D, D, tid, held);
    nan = put_row<XH>(a.x, xseq + (size_t)t0 * D, D, tid, held, xrow) || nan;
    const int32_t* pd = a.pdfs + (fseq + t0) * Kt;
    const float* pq = a.probs + (fseq + t0) * Kt;
    if constexpr (CLS) {
      class_table(c, pd, pq, Kt, D, tid, kSmNT, acl);
      __threadfence();
      __syncthreads();
      class_row_general(c.cls, hc, D, tid, acl, xrow, xacc);
    } else {
      for (int n = tid; n < D; n += kSmNT) xacc[n] = 0.f;
      __threadfence();
      __syncthreads();
      int d;
      float q;
      for (int k = tid; k < Kt; k += kSmNT)                                    // (scatter_entries, the row read around the L1)
        if (owned_entry(pd, pq, k, Kt, D, d, q)) xacc[d] = load_fresh(xrow + d) * q;
    }
    __threadfence();
    __syncthreads();
  }
  // frame j: forwards alpha'(t+1) from alpha'(t) and x(t), t = j; backwards beta'(t) from beta'(t+1) and x(t), t = L-1-j
  for (int j = 0; j < L; j++) {
    const int p = j & 1;
    const int t = FWD ? j : L - 1 - j, tn = FWD ? t + 1 : t - 1;
    const bool more = j + 1 < L;
    const int r = FWD ? t + 1 : t, rp = FWD ? t : t + 1;                       // the row made, the row it is made from
    float* const o0 = st0 + (size_t)r * H;
    float* const o1 = st1 + (size_t)r * H;
    const float* v0 = VLDS ? vec0 + (size_t)p * H : st0 + (size_t)rp * H;
    const float* v1 = VLDS ? vec1 + (size_t)p * H : st1 + (size_t)rp * H;
    float* w0 = VLDS ? vec0 + (size_t)(1 - p) * H : o0;                        // (raw sums wait in the row's own slot)
    float* w1 = VLDS ? vec1 + (size_t)(1 - p) * H : o1;
    const float* xr = xrow + (size_t)p * D;
    const float* xa = xacc + (size_t)p * D;
    float* xrn = xrow + (size_t)(1 - p) * D;
    float* xan = xacc + (size_t)(1 - p) * D;
    const int32_t* pd = a.pdfs + (fseq + (more ? tn : t)) * Kt;                // the next frame's entries
    const float* pq = a.probs + (fseq + (more ? tn : t)) * Kt;
    float held[kSmXR];
    if (more) hold_row<XH>(a.x, xseq + (size_t)tn * D, D, tid, held);          // the next frame's row: in flight over the arc loop
    if constexpr (CLS) {                                                       // (the table's readers are behind the last barrier)
      if (more) class_table(c, pd, pq, Kt, D, tid, kSmNT, acl);
    } else {
      for (int n = tid; n < D; n += kSmNT) xan[n] = 0.f;
    }
    const float e_t = a.frame_acc[fseq + t];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int i = tid; i < H; i += kSmNT) {
      float acc0 = 0.f, acc1 = 0.f;
      const int k1 = idx[2 * (size_t)i + 1];
      for (int k = idx[2 * (size_t)i]; k < k1; k++) {
        const int other = arc[3 * (size_t)k + (FWD ? 0 : 1)], n = arc[3 * (size_t)k + 2];
        const float w = pr[k];
        const float u0 = VLDS ? v0[other] : load_fresh(v0 + other), u1 = VLDS ? v1[other] : load_fresh(v1 + other);
        const float xx = load_fresh(xr + n), xq = load_fresh(xa + n);
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
    __threadfence();                                                           // (the next row, its zeroed companion, the table)
    block_sum3<kSmNT>(s0, s1, s2, red, tid);                                   // (its barrier: the next rows are whole)
    if constexpr (CLS) {
      if (more) class_row_general(c.cls, hc, D, tid, acl, xrn, xan);
    } else {
      if (more) {
        int d;
        float q;
        for (int k = tid; k < Kt; k += kSmNT)
          if (owned_entry(pd, pq, k, Kt, D, d, q)) xan[d] = load_fresh(xrn + d) * q;
      }
    }
    const float inv = 1.f / s0;
    if (!(s0 > 0.f) || !(inv > 0.f) || !(inv - inv == 0.f)) bad = true;
    if (tid == 0) totv[r] = s0;
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
      if constexpr (VLDS) { w0[i] = c0; w1[i] = c1; }
      o0[i] = c0; o1[i] = c1;
    }
    __threadfence();                                                           // (the companion row; !VLDS: the state rows)
    __syncthreads();
  }
  // a NaN in a live row of x (the clamp turns it into exp(-30): watched here, by the forward workgroup), a total that is not
  // positive and finite: the sequence is bad.  (Both workgroups of a sequence may store the same 1.)
  if (__syncthreads_or((bad || (FWD && nan)) ? 1 : 0) && tid == 0) a.seq_bad[b] = 1;
}

template <int XH, bool CLS, bool VLDS>
__global__ __launch_bounds__(kSmNT) void smbr_general_recursion_kernel(const SmbrArgs a, const SmbrClasses c, const SmbrGeneral s) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  float* scratch = s.rec + (size_t)blockIdx.x * s.rec_stride;
  if (blockIdx.x < (unsigned)a.B) smbr_general_recursion<XH, true, CLS, VLDS>(a, c, scratch, blockIdx.x, lds);
  else smbr_general_recursion<XH, false, CLS, VLDS>(a, c, scratch, blockIdx.x - a.B, lds);
}

// smbr_grad_kernel / smbr_class_grad_kernel with the state rows read where the recursions left them and the D-rows in scratch
template <int XH, bool CLS>
__global__ __launch_bounds__(kSmGNT) void smbr_general_grad_kernel(const SmbrArgs a, const SmbrClasses c, const SmbrGeneral s) {
  __shared__ float red[kSmRed];
  const int tid = threadIdx.x;
  const SmbrGraph& g = a.g;
  const int H = g.H, D = a.D, T = a.T, Kt = a.Kt;
  float* const gq = s.grad + (size_t)blockIdx.x * s.grad_stride;     // [D] x q0
  float* const gv = gq + D;                                          // [D] x (q1 - e q0), then + A x q0
  float* const acl = gv + D;                                         // [C] Acls of the frame (CLS)
  const float gscale = a.grad_scale_dev ? a.grad_scale * *a.grad_scale_dev : a.grad_scale;
  const int nblk = (T + kSmFrames - 1) / kSmFrames;
  const int items = a.B * nblk;
  for (int it = blockIdx.x; it < items; it += gridDim.x) {
    const int b = it / nblk, blk = it - b * nblk;
    const int L = seq_len(a.lengths, b, T);
    const size_t seq_rows = (size_t)b * (T + 1);
    const int t_begin = blk * kSmFrames, t_end = min(t_begin + kSmFrames, T);
    for (int t = t_begin; t < t_end; t++) {
      const size_t row = ((size_t)b * T + t) * D;
      if (t >= L) {                                                            // padding: exact zeros
        for (int n = tid; n < D; n += kSmGNT) row_store1<XH>(a.grad, row + n, 0.f);
        continue;
      }
      const size_t r0 = (seq_rows + t) * H, r1 = r0 + H;
      const float* const sa = a.al + r0;                                       // alpha'(t)
      const float* const sab = a.ab + r0;                                      // alpha-bar'(t)
      const float* const sb = a.be + r1;                                       // beta'(t+1)
      const float* const sbb = a.bb + r1;                                      // beta-bar'(t+1)
      const int32_t* pd = a.pdfs + ((size_t)b * T + t) * Kt;
      const float* pq = a.probs + ((size_t)b * T + t) * Kt;
      if constexpr (CLS) {
        class_table(c, pd, pq, Kt, D, tid, kSmGNT, acl);
        __threadfence();
        __syncthreads();
      }
      const float e_t = a.frame_acc[(size_t)b * T + t];
      float part = 0.f, none1 = 0.f, none2 = 0.f;
      for (int n = tid; n < D; n += kSmGNT) {
        const int k0 = g.pidx[n], k1 = g.pidx[n + 1];
        float q0 = 0.f, q1 = 0.f;
        for (int k = k0; k < k1; k++) {
          const int id = g.parc[k];
          const int src = g.ft[3 * (size_t)id], dst = g.ft[3 * (size_t)id + 1];
          const float w = g.fp[id];
          const float wa = w * sa[src];
          q0 += wa * sb[dst];
          q1 += (w * sab[src]) * sb[dst] + wa * sbb[dst];
        }
        float v0 = 0.f, v1 = 0.f;
        if (k0 != k1) {                                                        // a pdf no arc carries: its x is not read
          const float xx = clamp_exp(row_load1<XH>(a.x, row + n), kXExpClamp);
          v0 = xx * q0;
          v1 = xx * (q1 - e_t * q0);
          if constexpr (CLS) v1 += load_fresh(acl + c.cls[n]) * v0;            // (+ A x q0: the thread's own element)
        }
        gq[n] = v0; gv[n] = v1;
        part += v0;
        if constexpr (CLS) none1 += v1;
      }
      if constexpr (!CLS) __threadfence();                                     // (the entries' owners read other threads' elements)
      block_sum3<kSmGNT>(part, none1, none2, red, tid);
      float mean = none1;
      if constexpr (!CLS) {
        int d;
        float q;
        for (int k = tid; k < Kt; k += kSmGNT)
          if (owned_entry(pd, pq, k, Kt, D, d, q)) gv[d] = load_fresh(gv + d) + q * load_fresh(gq + d);
        __threadfence();
        __syncthreads();
        // the row's mean: a second sum, over the FINISHED elements (smbr_grad_kernel says why); its scratch is red[48 ..]
        mean = 0.f;
        for (int n = tid; n < D; n += kSmGNT) mean += load_fresh(gv + n);
        mean = wave_sum(mean);
        if ((tid & 63) == 0) red[48 + (tid >> 6)] = mean;
        __syncthreads();
        mean = 0.f;
        for (int w = 0; w < kSmGNT / 64; w++) mean += red[48 + w];               // (same order in every thread)
      }
      const float sc = gscale / part, inv = 1.f / part;
      if ((!(part > 0.f) || !(inv - inv == 0.f)) && tid == 0) smbr_condemn(a, b);    // (the host twin's check of the same divisor)
      const float eps = mean * inv;                                            // the row is centred by its own mean
      for (int n = tid; n < D; n += kSmGNT) {
        const bool carried = g.pidx[n] != g.pidx[n + 1];
        row_store1<XH>(a.grad, row + n, carried ? (load_fresh(gv + n) - eps * load_fresh(gq + n)) * sc : 0.f);
      }
      __syncthreads();                                                         // (red is free for the next frame)
    }
    // the sequence's first item closes it: the diagnostic sum_j alpha-bar'(L,j) final(j) / sum_j alpha'(L,j) final(j), and the
    // sequence's verdict
    if (blk == 0) {
      const size_t rL = (seq_rows + L) * H;
      float c0 = 0.f, c1 = 0.f, none = 0.f;
      for (int i = tid; i < H; i += kSmGNT) { c0 += a.al[rL + i] * g.fin[i]; c1 += a.ab[rL + i] * g.fin[i]; }
      block_sum3<kSmGNT>(c0, c1, none, red, tid);
      if (tid == 0) {
        const bool bad = a.seq_bad[b] != 0 || !(c0 > 0.f);                     // what the recursions found
        a.closing[b] = bad ? __builtin_nanf("") : c1 / c0;
        if (bad) smbr_condemn(a, b);
      }
      __syncthreads();                                                         // (red is free for the next item)
    }
  }
}

template <int XH, bool CLS, bool VLDS>
hipError_t launch_recursion(const SmbrArgs& a, const SmbrClasses& c, const SmbrGeneral& s, hipStream_t st) {
  const size_t lds = (kSmRed + (VLDS ? 4 * (size_t)a.g.H : 0)) * sizeof(float);
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(smbr_general_recursion_kernel<XH, CLS, VLDS>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((smbr_general_recursion_kernel<XH, CLS, VLDS>), dim3(2 * a.B), dim3(kSmNT), lds, st, a, c, s);
  return hipGetLastError();
}

template <int XH, bool CLS>
hipError_t launch_as(const SmbrArgs& a, const SmbrClasses& c, const SmbrGeneral& s, hipStream_t st) {
  const hipError_t e = s.state_lds ? launch_recursion<XH, CLS, true>(a, c, s, st) : launch_recursion<XH, CLS, false>(a, c, s, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((smbr_general_grad_kernel<XH, CLS>), dim3(s.grad_wgs), dim3(kSmGNT), 0, st, a, c, s);
  return hipGetLastError();
}

template <int XH>
hipError_t launch_dtype(const SmbrArgs& a, const SmbrClasses& c, const SmbrGeneral& s, hipStream_t st) {
  return c.cls ? launch_as<XH, true>(a, c, s, st) : launch_as<XH, false>(a, c, s, st);
}

size_t round64(size_t floats) { return (floats + 63) & ~size_t(63); }

}  // namespace

size_t smbr_general_lds(int H) { return (4 * (size_t)H + kSmRed) * sizeof(float) + kSmStaticLds; }
size_t smbr_general_rec_stride(int D, int C) { return round64(4 * (size_t)D + (size_t)C); }
size_t smbr_general_grad_stride(int D, int C) { return round64(2 * (size_t)D + (size_t)C); }
int smbr_general_grad_wgs(int B, int T) {
  const size_t items = (size_t)B * ((T + kSmFrames - 1) / kSmFrames);
  return (int)(items < (size_t)kSmbrGradMaxWgs ? items : (size_t)kSmbrGradMaxWgs);
}

hipError_t launch_smbr_general(const SmbrArgs& a, const SmbrClasses& c, const SmbrGeneral& s, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.seq_bad, 0, 2 * (size_t)a.B * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  if (a.x_half == kXF32) return launch_dtype<kXF32>(a, c, s, st);
  if (a.x_half == kXBf16) return launch_dtype<kXBf16>(a, c, s, st);
  return launch_dtype<kXF16>(a, c, s, st);
}

}  // namespace pychain_hip
