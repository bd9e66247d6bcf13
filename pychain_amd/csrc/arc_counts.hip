// arc_counts.hip - expected arc counts of the denominator's path distribution (include/pychain_hip.h: pychain_hip_den_arc_counts;
// DESIGN.md §3.29): with every arc probability p_k replaced by p_k exp(w_k),
//
//   c(b,k) = d log Z_b / d w_k = sum_t alpha'(t,src_k) p_k e^{w_k} x(t,pdf_k) beta'(t+1,dst_k) / (the same summed over the arcs at t)
//
// the arc-level form of the occupancy identity (§3.3): the E-step statistics of the graph, and the gradient of log Z_b in the
// arc log-weights.  The plan-compiled kernels bake the probabilities in, so this is a path of its own over the reference layout:
//
//   arc_weight_kernel      once per call: pw(k) = p_k exp(w_k) in the forward order and in the backward order (the backward copy of
//                          an arc finds its forward id by its endpoints, pdf and probability; arcs equal in all four pair up in
//                          order).  A weight that is not finite counts in bad_count[1] and is taken as 0.
//   arc_recursion_kernel   the `recursion` of smbr_device.h without its weighted pair (the body smbr_recursion_kernel runs with it;
//                          no instruction of the pair is left): 2B persistent workgroups, one per (sequence, direction),
//                          the state vector and the row x = exp(clamp(y)) double-buffered in LDS, the row made a frame ahead; a
//                          thread owns states tid, tid + 1024, ...; alpha' and beta', normalised per frame, go to the workspace
//                          with the totals divided out.
//   arc_count_kernel       time-parallel over (sequence, run of kArcFrames frames): alpha'(t) and beta'(t+1) in LDS, a thread owns
//                          pdfs tid, tid + 512, ... and walks that pdf's arcs through the caller's by-pdf order, twice: for the
//                          frame's divisor sum_n x(n) q0(n), then for the arc posteriors, which it adds to the workgroup's partial
//                          row [K] (fp64) in the workspace - every arc has one owner, so this is a plain read-modify-write - while
//                          gamma(t,n) = x(n) q0(n) / divisor is the thread's own sum and is stored once, in x's type.
//   arc_objf_kernel        log Z_b = sum_t log tot(t) + log sum_j alpha'(L,j) final(j) in fp64, and the sequence's verdict
//   arc_reduce_kernel      counts(k) = sum_b u_b sum_j partial(b,j,k): fp64, the workgroups of a sequence in ascending j, then the
//                          sequences in ascending b.  A sequence that went bad, or whose weight is 0, is left out.
// Nothing is atomic but integer counters; every sum has a fixed order, so a call gives the same bits every time.  Contraction is
// off for the whole unit, as in smbr.hip: the 2-byte forms compute what the fp32 form computes on the up-cast input.
// These kernels keep a frame in LDS and pychain_hip_den_arc_counts refuses what does not fit.  The GENERAL kernels (DESIGN.md
// §3.30; pychain_hip_den_arc_counts_general) take any graph and tree, as smbr_general.hip does for sMBR - SLOW: what does not fit
// LDS is gathered from global memory -, between the same launches before and behind:
//   arc_general_recursion_kernel<XH, VLDS>   the same `recursion` over FrameRows ("rows": the state vector double-buffered in LDS,
//                          2 H floats) or FrameGlobal ("global": the previous state row read back from the trajectory the workgroup
//                          has just written); the row x [2][D] lies in the workgroup's scratch row of the workspace.
//   arc_general_count_kernel<XH, VLDS>   at most kArcCountMaxWgs workgroups, persistent over the (sequence, run of kArcFrames
//                          frames) items, each frame by arc_count_frame, arc_count_kernel's loop body; the two D-rows a thread writes and reads
//                          back itself lie in the workgroup's scratch row, alpha'(t) and beta'(t+1) are staged in LDS ("rows") or
//                          gathered from the trajectories ("global": written by the launch before, plain loads).  The partial row
//                          stays the item's, so the reduction is the same.
// SAME BITS: ownership, the arc order and the order of every sum are those of the LDS kernels - the recursion is one copy
// (smbr_device.h), the count frame the LDS kernel's expressions in its order -, so where both run the general kernels give the
// bits of the LDS kernels (tests/test_gpu_arc_counts_general.py).
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

// 64 frames a count workgroup: at the benchmark shape (B = 64, T = 1500, K = 30000) 64 x 24 partial rows of 240 kB, 369 MB
constexpr int kArcFrames = 64;
constexpr int kArcNT = 256;                 // the small kernels

struct ArcArgs {
  SmbrGraph g;
  const float* lw;                       // [K] arc log-weights in the forward order, or null
  const void* x; int x_half;             // [B,T,D] raw
  const int64_t* lengths;
  const float* seq_w;                    // [B] or null
  float coef, grad_scale; const float* grad_scale_dev;
  void* grad;                            // [B,T,D] out in x's type, or null
  double* objf;                          // [B]
  double* counts;                        // [K]
  double* counts_per_seq;                // [B,K] or null
  int32_t* bad_count;                    // [2]
  float *pwf, *pwb;                      // workspace: [K] p exp(w) in the forward / in the backward order
  float *al, *be;                        // workspace: [B][T+1][H]
  float *tot_a, *tot_b;                  // workspace: [B][T+1]
  int32_t* seq_bad;                      // workspace: [3][B], zeroed: what the recursions found, the count frames, the verdict
  double* partial;                       // workspace: [B][nblk][K]
  int B, T, D, nblk;
};

// The general kernels' scratch rows in the workspace, behind the partial rows: what the LDS kernels keep in LDS beside the state
// vectors.  A recursion workgroup's row holds x [2][D], a count workgroup's x [D], x q0 [D].
struct ArcGeneral {
  float* rec;                            // [2 B][stride]
  float* cnt;                            // [cnt_wgs][stride]
  size_t stride;                         // floats, a multiple of 64
  int cnt_wgs;                           // workgroups of the count launch, persistent over the (sequence, run) items
  int state_lds;                         // 1: the state vectors in LDS ("rows"); 0: read back from the trajectories ("global")
};
constexpr int kArcCountMaxWgs = 512;     // two count workgroups a CU, as kSmbrGradMaxWgs: bounds the scratch

// ---- p exp(w) ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float arc_weighted(const float* lw, int id, float p, bool& bad) {
  if (!lw || id < 0) return p;
  const float w = lw[id];
  if (!(w - w == 0.f)) { bad = true; return p; }                               // NaN, +-inf: counted, taken as 0
  return p * expf(w);
}
__global__ __launch_bounds__(kArcNT) void arc_weight_kernel(const ArcArgs a) {
  const SmbrGraph& g = a.g;
  const int k = blockIdx.x * kArcNT + threadIdx.x;
  if (k >= g.K) return;
  bool bad = false, none = false;
  a.pwf[k] = arc_weighted(a.lw, k, g.fp[k], bad);
  if (bad) atomicAdd(a.bad_count + 1, 1);                                      // (an integer count)
  // the backward copy k of an arc: the r-th of its source's run with these endpoints, pdf and probability, r its rank among the
  // equal arcs of its destination's run
  const int src = g.bt[3 * k], dst = g.bt[3 * k + 1], pdf = g.bt[3 * k + 2];
  const float p = g.bp[k];
  int id = -1;
  if (a.lw && src >= 0 && src < g.H && dst >= 0 && dst < g.H) {
    int rank = 0;
    for (int j = max(g.bi[2 * dst], 0); j < k; j++)
      if (g.bt[3 * j] == src && g.bt[3 * j + 2] == pdf && g.bp[j] == p) rank++;
    const int j1 = min(g.fi[2 * src + 1], g.K);
    for (int j = max(g.fi[2 * src], 0); j < j1; j++)
      if (g.ft[3 * j + 1] == dst && g.ft[3 * j + 2] == pdf && g.fp[j] == p && rank-- == 0) { id = j; break; }
  }
  a.pwb[k] = arc_weighted(a.lw, id, p, none);
}

// ---- the recursions ---------------------------------------------------------------------------------------------------------------
// `recursion` (smbr_device.h) without the weighted pair, over FrameLds, on the weighted probabilities.  LDS: [2][H] alpha' / beta',
// [2][D] x, the reduction scratch
template <int XH>
__global__ __launch_bounds__(kSmNT) void arc_recursion_kernel(const ArcArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  RecArgs r{a.g};
  r.pf = a.pwf; r.pb = a.pwb; r.x = a.x; r.lengths = a.lengths; r.coef = a.coef;
  r.al = a.al; r.be = a.be; r.tot_a = a.tot_a; r.tot_b = a.tot_b; r.seq_bad = a.seq_bad; r.T = a.T; r.D = a.D;
  r.vec0 = lds; r.xrow = r.vec0 + 2 * (size_t)a.g.H; r.red = r.xrow + 2 * (size_t)a.D;
  if (blockIdx.x < (unsigned)a.B) recursion<XH, true, false, false, FrameLds>(r, SmbrClasses{}, blockIdx.x);
  else recursion<XH, false, false, false, FrameLds>(r, SmbrClasses{}, blockIdx.x - a.B);
}
// ... over FrameRows (VLDS) or FrameGlobal: x [2][D] in the workgroup's scratch row; LDS: the reduction scratch, then with VLDS
// [2][H] alpha' / beta'
template <int XH, bool VLDS>
__global__ __launch_bounds__(kSmNT) void arc_general_recursion_kernel(const ArcArgs a, const ArcGeneral s) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  using S = std::conditional_t<VLDS, FrameRows, FrameGlobal>;
  RecArgs r{a.g};
  r.pf = a.pwf; r.pb = a.pwb; r.x = a.x; r.lengths = a.lengths; r.coef = a.coef;
  r.al = a.al; r.be = a.be; r.tot_a = a.tot_a; r.tot_b = a.tot_b; r.seq_bad = a.seq_bad; r.T = a.T; r.D = a.D;
  r.red = lds; r.vec0 = lds + kSmRed; r.xrow = s.rec + (size_t)blockIdx.x * s.stride;
  if (blockIdx.x < (unsigned)a.B) recursion<XH, true, false, false, S>(r, SmbrClasses{}, blockIdx.x);
  else recursion<XH, false, false, false, S>(r, SmbrClasses{}, blockIdx.x - a.B);
}

// ---- the counts -------------------------------------------------------------------------------------------------------------------
template <int XH>
__global__ __launch_bounds__(kSmGNT) void arc_count_kernel(const ArcArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  const int tid = threadIdx.x, b = blockIdx.y;
  const SmbrGraph& g = a.g;
  const int H = g.H, D = a.D, T = a.T;
  const int L = seq_len(a.lengths, b, T);
  float* const sa = lds;                          // alpha'(t)
  float* const sb = sa + H;                       // beta'(t+1)
  float* const gx = sb + H;                       // [D] x
  float* const gq = gx + D;                       // [D] x q0
  float* const red = gq + D;
  const size_t seq_rows = (size_t)b * (T + 1);
  float gscale = a.grad_scale_dev ? a.grad_scale * *a.grad_scale_dev : a.grad_scale;
  if (a.seq_w) gscale = gscale * a.seq_w[b];
  double* const prow = a.partial + ((size_t)b * a.nblk + blockIdx.x) * g.K;    // (written from the first live frame on: read by
  bool first = true;                                                           // the reduction only where the run has one)
  const int t_begin = blockIdx.x * kArcFrames, t_end = min(t_begin + kArcFrames, T);
  for (int t = t_begin; t < t_end; t++) {
    const size_t row = ((size_t)b * T + t) * D;
    if (t >= L) {                                                              // padding: exact zeros
      if (a.grad)
        for (int n = tid; n < D; n += kSmGNT) row_store1<XH>(a.grad, row + n, 0.f);
      continue;
    }
    const size_t r0 = (seq_rows + t) * H, r1 = r0 + H;
    for (int i = tid; i < H; i += kSmGNT) { sa[i] = a.al[r0 + i]; sb[i] = a.be[r1 + i]; }
    __syncthreads();
    float part = 0.f, none1 = 0.f, none2 = 0.f;
    for (int n = tid; n < D; n += kSmGNT) {
      const int k0 = g.pidx[n], k1 = g.pidx[n + 1];
      float q0 = 0.f;
      for (int k = k0; k < k1; k++) {
        const int id = g.parc[k];
        q0 += (a.pwf[id] * sa[g.ft[3 * id]]) * sb[g.ft[3 * id + 1]];
      }
      float xx = 0.f, v0 = 0.f;
      if (k0 != k1) {                                                          // a pdf no arc carries: its x is not read
        xx = clamp_exp(row_load1<XH>(a.x, row + n), kXExpClamp);
        v0 = xx * q0;
      }
      gx[n] = xx; gq[n] = v0;                                                  // (read back by this thread alone)
      part += v0;
    }
    block_sum3<kSmGNT>(part, none1, none2, red, tid);
    const float inv = 1.f / part, sc = gscale / part;
    if ((!(part > 0.f) || !(inv - inv == 0.f)) && tid == 0) a.seq_bad[a.B + b] = 1;      // (the same 1 whoever stores it)
    for (int n = tid; n < D; n += kSmGNT) {
      const int k0 = g.pidx[n], k1 = g.pidx[n + 1];
      if (a.grad) row_store1<XH>(a.grad, row + n, k0 != k1 ? gq[n] * sc : 0.f);
      const float xs = gx[n] * inv;
      for (int k = k0; k < k1; k++) {
        const int id = g.parc[k];
        const float post = ((a.pwf[id] * sa[g.ft[3 * id]]) * sb[g.ft[3 * id + 1]]) * xs;
        prow[id] = first ? (double)post : prow[id] + (double)post;             // the arc's one owner
      }
    }
    first = false;
    __syncthreads();                                                           // (the rows are free for the next frame)
  }
}

// The general form of a frame of arc_count_kernel, LINE FOR LINE its loop body - the same expressions in the same order, so the
// same bits - over the storage policy S of smbr_device.h.  (The LDS kernel does not call it: routed through this function its
// scalar address arithmetic compiles differently, and its device code is kept the one that was measured.)
// Frame t of sequence b (of L frames) into the partial row `prow` [K] of its run, by a workgroup of kSmGNT threads; true where the
// frame is live.  `first`: no live frame of the run has stored yet - the row is written from the first live frame on (read by the
// reduction only where the run has one).  alpha'(t) and beta'(t+1) are staged in `stage` [2][H] (S::kVecLds) or read where the
// recursion launch left them; gx, gq [D] are LDS or a scratch row of the workspace: each element is read back by the thread that
// wrote it, so neither needs a fence.  `red` is free again behind the frame's closing barrier.
template <int XH, class S>
__device__ __forceinline__ bool arc_count_frame(const ArcArgs& a, int b, size_t seq_rows, int t, int L, float gscale, double* prow, bool first,
                                                float* stage, float* gx, float* gq, float* red) {
  using Index = typename S::Index;
  const int tid = threadIdx.x;
  const SmbrGraph& g = a.g;
  const int H = g.H, D = a.D, T = a.T;
  const size_t row = ((size_t)b * T + t) * D;
  if (t >= L) {                                                                // padding: exact zeros
    if (a.grad)
      for (int n = tid; n < D; n += kSmGNT) row_store1<XH>(a.grad, row + n, 0.f);
    return false;
  }
  const size_t r0 = (seq_rows + t) * H, r1 = r0 + H;
  float* const stage1 = stage + H;
  const float* const sa = S::kVecLds ? stage : a.al + r0;                      // alpha'(t)
  const float* const sb = S::kVecLds ? stage1 : a.be + r1;                     // beta'(t+1)
  if constexpr (S::kVecLds) {
    for (int i = tid; i < H; i += kSmGNT) { stage[i] = a.al[r0 + i]; stage1[i] = a.be[r1 + i]; }
    __syncthreads();
  }
  float part = 0.f, none1 = 0.f, none2 = 0.f;
  for (int n = tid; n < D; n += kSmGNT) {
    const int k0 = g.pidx[n], k1 = g.pidx[n + 1];
    float q0 = 0.f;
    for (int k = k0; k < k1; k++) {
      const int id = g.parc[k];
      q0 += (a.pwf[id] * sa[g.ft[3 * (Index)id]]) * sb[g.ft[3 * (Index)id + 1]];
    }
    float xx = 0.f, v0 = 0.f;
    if (k0 != k1) {                                                            // a pdf no arc carries: its x is not read
      xx = clamp_exp(row_load1<XH>(a.x, row + n), kXExpClamp);
      v0 = xx * q0;
    }
    gx[n] = xx; gq[n] = v0;                                                    // (read back by this thread alone)
    part += v0;
  }
  block_sum3<kSmGNT>(part, none1, none2, red, tid);
  const float inv = 1.f / part, sc = gscale / part;
  if ((!(part > 0.f) || !(inv - inv == 0.f)) && tid == 0) a.seq_bad[a.B + b] = 1;        // (the same 1 whoever stores it)
  for (int n = tid; n < D; n += kSmGNT) {
    const int k0 = g.pidx[n], k1 = g.pidx[n + 1];
    if (a.grad) row_store1<XH>(a.grad, row + n, k0 != k1 ? gq[n] * sc : 0.f);
    const float xs = gx[n] * inv;
    for (int k = k0; k < k1; k++) {
      const int id = g.parc[k];
      const float post = ((a.pwf[id] * sa[g.ft[3 * (Index)id]]) * sb[g.ft[3 * (Index)id + 1]]) * xs;
      prow[id] = first ? (double)post : prow[id] + (double)post;               // the arc's one owner
    }
  }
  __syncthreads();                                                             // (the rows and red are free for the next frame)
  return true;
}

// at most kArcCountMaxWgs workgroups, persistent over the items it = b * nblk + run, whose partial row is row `it` - the run
// count the reduction derives from a length is the LDS launch's.  gx, gq in the workgroup's scratch row; LDS: the reduction
// scratch, then with VLDS the two state rows [2][H]
template <int XH, bool VLDS>
__global__ __launch_bounds__(kSmGNT) void arc_general_count_kernel(const ArcArgs a, const ArcGeneral s) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* const red = reinterpret_cast<float*>(smem_raw);
  using S = std::conditional_t<VLDS, FrameRows, FrameGlobal>;
  float* const gx = s.cnt + (size_t)blockIdx.x * s.stride;
  float* const gq = gx + a.D;
  const int items = a.B * a.nblk;                                              // (B * (T + 1) fits an int: checked by the host)
  for (int it = blockIdx.x; it < items; it += gridDim.x) {
    const int b = it / a.nblk, run = it - b * a.nblk;
    const int L = seq_len(a.lengths, b, a.T);
    const size_t seq_rows = (size_t)b * (a.T + 1);
    float gscale = a.grad_scale_dev ? a.grad_scale * *a.grad_scale_dev : a.grad_scale;
    if (a.seq_w) gscale = gscale * a.seq_w[b];
    double* const prow = a.partial + (size_t)it * a.g.K;
    bool first = true;                                                         // (per item)
    const int t_begin = run * kArcFrames, t_end = min(t_begin + kArcFrames, a.T);
    for (int t = t_begin; t < t_end; t++)
      if (arc_count_frame<XH, S>(a, b, seq_rows, t, L, gscale, prow, first, red + kSmRed, gx, gq, red)) first = false;
  }
}

// ---- log Z_b and the verdict ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kArcNT) void arc_objf_kernel(const ArcArgs a) {
  __shared__ double red[2][kArcNT / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int H = a.g.H, L = seq_len(a.lengths, b, a.T);
  const size_t seq_rows = (size_t)b * (a.T + 1);
  double lz = 0.0, c0 = 0.0;
  for (int t = tid; t <= L; t += kArcNT) lz += log((double)a.tot_a[seq_rows + t]);
  const float* aL = a.al + (seq_rows + L) * H;
  for (int i = tid; i < H; i += kArcNT) c0 += (double)aL[i] * (double)a.g.fin[i];
  lz = wave_sum_f64(lz); c0 = wave_sum_f64(c0);
  if ((tid & 63) == 0) { red[0][tid >> 6] = lz; red[1][tid >> 6] = c0; }
  __syncthreads();
  if (tid == 0) {
    lz = 0.0; c0 = 0.0;
    for (int w = 0; w < kArcNT / 64; w++) { lz += red[0][w]; c0 += red[1][w]; }
    lz += log(c0);
    const bool bad = a.seq_bad[b] != 0 || a.seq_bad[a.B + b] != 0 || !(c0 > 0.0) || !(lz - lz == 0.0);
    a.seq_bad[2 * a.B + b] = bad ? 1 : 0;
    a.objf[b] = bad ? __builtin_nan("") : lz;
    if (bad) atomicAdd(a.bad_count, 1);                                        // (an integer count; once per sequence)
  }
}

// ---- the sums -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kArcNT) void arc_reduce_kernel(const ArcArgs a) {
  const int K = a.g.K;
  const int k = blockIdx.x * kArcNT + threadIdx.x;
  if (k >= K) return;
  double total = 0.0;
  for (int b = 0; b < a.B; b++) {
    double s = 0.0;
    if (!a.seq_bad[2 * a.B + b]) {
      const int runs = (seq_len(a.lengths, b, a.T) + kArcFrames - 1) / kArcFrames;
      const double* p = a.partial + (size_t)b * a.nblk * K + k;
      for (int j = 0; j < runs; j++) s += p[(size_t)j * K];
      const float u = a.seq_w ? a.seq_w[b] : 1.f;
      if (u != 0.f) total += (double)u * s;
    }
    if (a.counts_per_seq) a.counts_per_seq[(size_t)b * K + k] = s;
  }
  a.counts[k] = total;
}

// both kernels: two state vectors, two rows, the reduction scratch
size_t arc_kernel_lds(int H, int D) { return (2 * (size_t)H + 2 * (size_t)D + kSmRed) * sizeof(float); }
size_t arc_lds_bytes(int H, int D) { return arc_kernel_lds(H, D) + kSmStaticLds; }       // (the recursion's static LDS)
// the general kernels: the reduction scratch, and under "rows" one double-buffered state vector (the recursion) or two state rows
// (the counts)
size_t arc_general_kernel_lds(int H, bool state_lds) { return (kSmRed + (state_lds ? 2 * (size_t)H : 0)) * sizeof(float); }
size_t arc_general_lds_bytes(int H) { return arc_general_kernel_lds(H, true) + kSmStaticLds; }

// the recursion launch and the count launch of a general form
template <int XH, bool VLDS>
hipError_t launch_arc_general(const ArcArgs& a, const ArcGeneral& s, hipStream_t st) {
  const size_t lds = arc_general_kernel_lds(a.g.H, VLDS);
  const hipError_t e = launch_with_lds(arc_general_recursion_kernel<XH, VLDS>, dim3(2 * a.B), dim3(kSmNT), lds, st, a, s);
  if (e != hipSuccess) return e;
  return launch_with_lds(arc_general_count_kernel<XH, VLDS>, dim3(s.cnt_wgs), dim3(kSmGNT), lds, st, a, s);
}

// `s` null: the LDS kernels
hipError_t launch_arc_counts(const ArcArgs& a, const ArcGeneral* s, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.seq_bad, 0, 3 * (size_t)a.B * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.bad_count, 0, 2 * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  const int kgrid = (a.g.K + kArcNT - 1) / kArcNT;
  hipLaunchKernelGGL(arc_weight_kernel, dim3(kgrid), dim3(kArcNT), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (!s)
    e = by_row_dtype(a.x_half, [&](auto xh) {
      constexpr int XH = decltype(xh)::value;
      const size_t lds = arc_kernel_lds(a.g.H, a.D);
      const hipError_t er = launch_with_lds(arc_recursion_kernel<XH>, dim3(2 * a.B), dim3(kSmNT), lds, st, a);
      if (er != hipSuccess) return er;
      return launch_with_lds(arc_count_kernel<XH>, dim3(a.nblk, a.B), dim3(kSmGNT), lds, st, a);
    });
  else
    e = by_row_dtype(a.x_half, [&](auto xh) {
      constexpr int XH = decltype(xh)::value;
      return s->state_lds ? launch_arc_general<XH, true>(a, *s, st) : launch_arc_general<XH, false>(a, *s, st);
    });
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(arc_objf_kernel, dim3(a.B), dim3(kArcNT), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(arc_reduce_kernel, dim3(kgrid), dim3(kArcNT), 0, st, a);
  return hipGetLastError();
}

struct ArcCarve { size_t al, be, tot_a, tot_b, seq_bad, pwf, pwb, partial, end, total; int nblk; };
ArcCarve arc_carve(int B, int T, int H, int K) {
  ArcCarve c;
  const size_t traj = align256((size_t)B * (T + 1) * H * sizeof(float)), tot = align256((size_t)B * (T + 1) * sizeof(float));
  const size_t pw = align256((size_t)K * sizeof(float));
  c.nblk = (T + kArcFrames - 1) / kArcFrames;
  size_t o = 0;
  c.al = o; o += traj; c.be = o; o += traj;
  c.tot_a = o; o += tot; c.tot_b = o; o += tot;
  c.seq_bad = o; o += align256(3 * (size_t)B * sizeof(int32_t));
  c.pwf = o; o += pw; c.pwb = o; o += pw;
  c.partial = o; o += align256((size_t)B * c.nblk * K * sizeof(double));
  c.end = o;
  c.total = o + 256;                               // (the base is aligned inside the caller's buffer)
  return c;
}
// the general kernels' scratch rows (ArcGeneral) behind the layout above, which they keep
struct ArcGeneralCarve { size_t rec, cnt, total; ArcGeneral s; };
ArcGeneralCarve arc_general_carve(const ArcCarve& c, int B, int D) {
  ArcGeneralCarve v;
  memset(&v, 0, sizeof(v));
  v.s.stride = (2 * (size_t)D + 63) & ~size_t(63);
  const size_t items = (size_t)B * c.nblk;
  v.s.cnt_wgs = (int)(items < (size_t)kArcCountMaxWgs ? items : (size_t)kArcCountMaxWgs);
  size_t o = c.end;
  v.rec = o; o += align256(2 * (size_t)B * v.s.stride * sizeof(float));
  v.cnt = o; o += align256((size_t)v.s.cnt_wgs * v.s.stride * sizeof(float));
  v.total = o + 256;
  return v;
}

// The form a call of the general entry point runs (include/pychain_hip.h: PYCHAIN_HIP_SMBR_*), or a negative code with the
// message set.
int arc_resolve_form(const char* who, int H, int D, int requested) {
  if (H <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes H=%d D=%d", who, H, D);
  if (requested < PYCHAIN_HIP_SMBR_AUTO || requested > PYCHAIN_HIP_SMBR_GLOBAL)
    return fail(PYCHAIN_HIP_EINVAL, "%s: unknown form %d (PYCHAIN_HIP_SMBR_AUTO .. _GLOBAL)", who, requested);
  const size_t lds = arc_lds_bytes(H, D), rows = arc_general_lds_bytes(H);
  if (requested == PYCHAIN_HIP_SMBR_LDS && lds > kSmbrLdsBudget)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: the LDS form needs %zu bytes of LDS for %d states and %d pdfs (two state vectors and two rows), a CU has %zu",
                who, lds, H, D, kSmbrLdsBudget);
  if (requested == PYCHAIN_HIP_SMBR_ROWS && rows > kSmbrLdsBudget)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: the rows form needs %zu bytes of LDS for %d states (one double-buffered state vector), a CU has %zu",
                who, rows, H, kSmbrLdsBudget);
  if (requested != PYCHAIN_HIP_SMBR_AUTO) return requested;
  return lds <= kSmbrLdsBudget ? PYCHAIN_HIP_SMBR_LDS : rows <= kSmbrLdsBudget ? PYCHAIN_HIP_SMBR_ROWS : PYCHAIN_HIP_SMBR_GLOBAL;
}
constexpr int kArcFormOfOld = -1;                  // the entry point from before the general kernels: LDS or refused, its message

// both entry points
int den_arc_counts(
    const char* who,
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const float* arc_log_weights, const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    float leaky_hmm_coefficient, const float* seq_weights, float grad_scale, const float* grad_scale_dev,
    void* grad, double* objf_per_seq, double* counts, double* counts_per_seq, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream, int form) {
  const NumGraphs graphs{ft, fi, fp, bt, bi, bp, initial, final_, 0, H, num_arcs};
  const Rows rows{nnet_output, nnet_output_dtype, seq_lengths, B, T, D};
  int rc = bad_dtype(who, nnet_output_dtype);
  if (rc != PYCHAIN_HIP_OK) return rc;
  if (graphs.any_null() || !leaky || !pdf_arcs || !pdf_index || !rows.x || !rows.lengths || !objf_per_seq || !counts || !bad_count || !workspace)
    return null_pointer(who);
  if ((rc = bad_sizes(who, rows, graphs)) != PYCHAIN_HIP_OK) return rc;
  if (!(leaky_hmm_coefficient > 0.f && leaky_hmm_coefficient < 1.f))
    return fail(PYCHAIN_HIP_EINVAL, "%s: leaky_hmm_coefficient must be in (0,1), got %g", who, (double)leaky_hmm_coefficient);
  int run = PYCHAIN_HIP_SMBR_LDS;
  if (form == kArcFormOfOld) {
    const size_t lds = arc_lds_bytes(H, D);
    if (lds > kSmbrLdsBudget)
      return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: %d states and %d pdfs need %zu bytes of LDS (two state vectors and two rows), a CU has %zu",
                  who, H, D, lds, kSmbrLdsBudget);
  } else if ((run = arc_resolve_form(who, H, D, form)) < 0) {
    return run;
  }
  if ((size_t)B * (T + 1) > (size_t)INT_MAX) return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: B * (T + 1) = %zu rows", who, (size_t)B * (T + 1));
  const ArcCarve c = arc_carve(B, T, H, num_arcs);
  ArcGeneralCarve gc = arc_general_carve(c, B, D);
  const size_t ws_need = run == PYCHAIN_HIP_SMBR_LDS ? c.total : gc.total;     // (the LDS form takes the present carve alone)
  if (workspace_bytes < ws_need) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, ws_need);
  char* base = ws_base(workspace);
  ArcArgs a;
  memset(&a, 0, sizeof(a));
  a.g = SmbrGraph{ft, fi, fp, bt, bi, bp, leaky, initial, final_, pdf_arcs, pdf_index, H, num_arcs};
  a.lw = arc_log_weights; a.x = nnet_output; a.x_half = nnet_output_dtype; a.lengths = seq_lengths; a.seq_w = seq_weights;
  a.coef = leaky_hmm_coefficient; a.grad_scale = grad_scale; a.grad_scale_dev = grad_scale_dev;
  a.grad = grad; a.objf = objf_per_seq; a.counts = counts; a.counts_per_seq = counts_per_seq; a.bad_count = bad_count;
  a.pwf = (float*)(base + c.pwf); a.pwb = (float*)(base + c.pwb);
  a.al = (float*)(base + c.al); a.be = (float*)(base + c.be);
  a.tot_a = (float*)(base + c.tot_a); a.tot_b = (float*)(base + c.tot_b); a.seq_bad = (int32_t*)(base + c.seq_bad);
  a.partial = (double*)(base + c.partial);
  a.B = B; a.T = T; a.D = D; a.nblk = c.nblk;
  gc.s.rec = (float*)(base + gc.rec); gc.s.cnt = (float*)(base + gc.cnt);
  gc.s.state_lds = run == PYCHAIN_HIP_SMBR_ROWS;
  const hipError_t err = launch_arc_counts(a, run == PYCHAIN_HIP_SMBR_LDS ? nullptr : &gc.s, (hipStream_t)stream);
  if (err != hipSuccess) return launch_failed(who, err, nullptr);
  return PYCHAIN_HIP_OK;
}

}  // namespace
}  // namespace pychain_hip

using namespace pychain_hip;

// ---- the entry points (include/pychain_hip.h) -----------------------------------------------------------------------------------
extern "C" size_t pychain_hip_den_arc_counts_workspace_bytes(int B, int T, int H, int num_arcs) {
  if (B <= 0 || T <= 0 || H <= 0 || num_arcs <= 0) return 0;
  return arc_carve(B, T, H, num_arcs).total;
}

extern "C" size_t pychain_hip_den_arc_counts_lds_bytes(int H, int D) {
  if (H <= 0 || D <= 0) return 0;
  return arc_lds_bytes(H, D);
}

extern "C" size_t pychain_hip_den_arc_counts_general_lds_bytes(int H) {
  if (H <= 0) return 0;
  return arc_general_lds_bytes(H);
}

extern "C" int pychain_hip_den_arc_counts_form(int H, int D, int requested) {
  return arc_resolve_form("den_arc_counts_form", H, D, requested);
}

extern "C" size_t pychain_hip_den_arc_counts_general_workspace_bytes(int B, int T, int H, int num_arcs, int D) {
  if (B <= 0 || T <= 0 || H <= 0 || num_arcs <= 0 || D <= 0) return 0;
  return arc_general_carve(arc_carve(B, T, H, num_arcs), B, D).total;
}

extern "C" int pychain_hip_den_arc_counts(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const float* arc_log_weights, const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    float leaky_hmm_coefficient, const float* seq_weights, float grad_scale, const float* grad_scale_dev,
    void* grad, double* objf_per_seq, double* counts, double* counts_per_seq, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream) {
  return den_arc_counts("den_arc_counts", ft, fi, fp, bt, bi, bp, leaky, initial, final_, pdf_arcs, pdf_index, H, num_arcs, arc_log_weights,
                        nnet_output, nnet_output_dtype, seq_lengths, B, T, D, leaky_hmm_coefficient, seq_weights, grad_scale, grad_scale_dev,
                        grad, objf_per_seq, counts, counts_per_seq, bad_count, workspace, workspace_bytes, stream, kArcFormOfOld);
}

// any num_states and num_pdfs: `form` picks the kernels, PYCHAIN_HIP_SMBR_LDS today's launches
extern "C" int pychain_hip_den_arc_counts_general(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const float* arc_log_weights, const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    float leaky_hmm_coefficient, const float* seq_weights, float grad_scale, const float* grad_scale_dev,
    void* grad, double* objf_per_seq, double* counts, double* counts_per_seq, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream, int form) {
  if (form < PYCHAIN_HIP_SMBR_AUTO || form > PYCHAIN_HIP_SMBR_GLOBAL)
    return fail(PYCHAIN_HIP_EINVAL, "den_arc_counts_general: unknown form %d (PYCHAIN_HIP_SMBR_AUTO .. _GLOBAL)", form);
  return den_arc_counts("den_arc_counts_general", ft, fi, fp, bt, bi, bp, leaky, initial, final_, pdf_arcs, pdf_index, H, num_arcs, arc_log_weights,
                        nnet_output, nnet_output_dtype, seq_lengths, B, T, D, leaky_hmm_coefficient, seq_weights, grad_scale, grad_scale_dev,
                        grad, objf_per_seq, counts, counts_per_seq, bad_count, workspace, workspace_bytes, stream, form);
}
