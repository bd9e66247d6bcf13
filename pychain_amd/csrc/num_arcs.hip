// num_arcs.hip - expected arc counts of the NUMERATOR's path distribution (include/pychain_hip.h: pychain_hip_num_arc_counts;
// DESIGN.md §3.31): with every arc log-probability lp_k of sequence b's graph replaced by lp_k + w(b,k),
//
//   c(b,k) = d log P_b / d w(b,k) = sum_{t < L_b} exp(alpha'(t,src_k) + lp_k + w(b,k) + x(t,pdf_k) + beta'(t+1,dst_k) - log P_b)
//
// The recursions and the occupancy pass are the launches of num_kernels.hip / num_general.hip, given other probability buffers;
// their backward pass leaves every forward arc's log-share r_k(t) (NumArgs::frac_ws), so the posterior of arc k at frame t is
// exp(alpha'(t,src_k) + beta'(t,src_k) - log P_b + r_k(t)) and this unit needs neither the network output nor the weights again:
//
//   num_arc_weight_kernel   once per call, only with weights: fl32(lp_k + w(b,k)) in the forward order and in the backward order
//                           [B,K] (the backward copy of an arc finds its forward id by its endpoints, pdf and log-probability;
//                           arcs equal in all four pair up in order - arc_weight_kernel's rule, within the sequence's used
//                           arcs).  A weight that is not finite counts in bad_count[1] and is taken as 0; padding arcs are not
//                           read.  For a shared graph it also copies the transition, index, initial and final arrays once per
//                           sequence: the recursion kernels have one stride for all of a graph's arrays.
//   num_arc_count_kernel    time-parallel, a workgroup per (sequence, run of kNumArcFrames frames), every arc with one owner
//                           thread: st = fl32(alpha + beta - log P) of the source state (formed in fp64, rounded once, as
//                           num_occ_kernel), post = fexp(st + r_k(t)) in fp32, summed over the run's frames in fp64 in ascending t
//                           into the run's partial row [K] with plain stores.  STAGED: the frame's st row [H] in LDS, frames
//                           outer; gathered: arcs outer, the two trajectory elements read per (arc, frame).  The same
//                           expressions in the same order: the same bits.
//   num_arc_reduce_kernel   counts(b,k) = the sequence's partial rows in ascending run (fp64); objf(b) = log P_b.  A sequence
//                           whose log P_b is not finite gets exact zeros.
// Nothing is atomic but integer counters (the used-arc maximum in LDS, the bad-weight count); every sum has a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)      // ahead of the project's headers, as arc_counts.hip

#include "../../include/pychain_hip.h"
#include "common.h"
#include "device_utils.h"
#include "num_arcs.h"

namespace pychain_hip {
namespace {

constexpr int kNaNT = 256;
constexpr int kNaReg = 4;                  // arcs a thread of the staged form sums in registers; further ones in the partial row
constexpr size_t kNaStageBudget = 48 * 1024;       // H <= 12288: within the 64 KiB a launch gets without asking, several workgroups a CU
constexpr float kNaLog2e = 1.44269504088896340736f;

__device__ __forceinline__ float na_exp(float d) { return __builtin_amdgcn_exp2f(d * kNaLog2e); }     // num_kernels.hip: fexp

// the largest end of a state's arc run: the sequence's used arcs are k < this (batch padding lies behind)
__device__ __forceinline__ int used_arcs(const int32_t* idx, int H, int K, int* s_max, int tid) {
  int kmax = 0;
  for (int h = tid; h < H; h += kNaNT) kmax = max(kmax, idx[2 * (size_t)h + 1]);
  if (tid == 0) *s_max = 0;
  __syncthreads();
  atomicMax(s_max, kmax);                  // (an integer, in LDS)
  __syncthreads();
  const int used = min(*s_max, K);
  __syncthreads();                         // (s_max may be used again)
  return used;
}

__global__ __launch_bounds__(kNaNT) void num_arc_weight_kernel(const NumArcWeightArgs a) {
  __shared__ int s_max;
  const int tid = threadIdx.x, b = blockIdx.y;
  const int H = a.H, K = a.K;
  const size_t g = (size_t)b * a.graph_stride;
  const int32_t* ft = a.ft + g * K * 3; const int32_t* fi = a.fi + g * H * 2; const float* fp = a.fp + g * K;
  const int32_t* bt = a.bt + g * K * 3; const int32_t* bi = a.bi + g * H * 2; const float* bp = a.bp + g * K;
  const float* w = a.w + (size_t)b * K;
  const int Kf = used_arcs(fi, H, K, &s_max, tid);
  const int Kb = used_arcs(bi, H, K, &s_max, tid);
  const int k = blockIdx.x * kNaNT + tid;
  if (a.rft) {                             // a shared graph: this sequence's copy of what the probabilities are indexed with
    if (k < K) {
      for (int i = 0; i < 3; i++) {
        a.rft[((size_t)b * K + k) * 3 + i] = ft[(size_t)3 * k + i];
        a.rbt[((size_t)b * K + k) * 3 + i] = bt[(size_t)3 * k + i];
      }
    }
    if (blockIdx.x == 0)
      for (int h = tid; h < H; h += kNaNT) {
        a.rfi[((size_t)b * H + h) * 2] = fi[2 * (size_t)h]; a.rfi[((size_t)b * H + h) * 2 + 1] = fi[2 * (size_t)h + 1];
        a.rbi[((size_t)b * H + h) * 2] = bi[2 * (size_t)h]; a.rbi[((size_t)b * H + h) * 2 + 1] = bi[2 * (size_t)h + 1];
        a.rinit[(size_t)b * H + h] = a.initial[g * H + h];
        a.rfin[(size_t)b * H + h] = a.final_[g * H + h];
      }
  }
  if (k >= K) return;
  // the forward order
  float vf = 0.f;                          // (padding arcs: neither the graph's nor the caller's entry is read)
  if (k < Kf) {
    float wk = w[k];
    if (!(wk - wk == 0.f)) { atomicAdd(a.bad, 1); wk = 0.f; }                  // NaN, +-inf: counted (an integer), taken as 0
    vf = fp[k] + wk;
  }
  a.wf[(size_t)b * K + k] = vf;
  // the backward copy k of an arc: the r-th of its source's run with these endpoints, pdf and log-probability, r its rank among
  // the equal arcs of its destination's run
  float vb = 0.f;
  if (k < Kb) {
    const int src = bt[(size_t)3 * k], dst = bt[(size_t)3 * k + 1], pdf = bt[(size_t)3 * k + 2];
    const float p = bp[k];
    vb = p;
    if (src >= 0 && src < H && dst >= 0 && dst < H) {
      int rank = 0;
      for (int j = max(bi[2 * (size_t)dst], 0); j < k; j++)
        if (bt[(size_t)3 * j] == src && bt[(size_t)3 * j + 2] == pdf && bp[j] == p) rank++;
      const int j1 = min(fi[2 * (size_t)src + 1], Kf);
      for (int j = max(fi[2 * (size_t)src], 0); j < j1; j++)
        if (ft[(size_t)3 * j + 1] == dst && ft[(size_t)3 * j + 2] == pdf && fp[j] == p && rank-- == 0) {
          const float wj = w[j];
          if (wj - wj == 0.f) vb = p + wj;                                     // (counted once, in the forward order)
          break;
        }
    }
  }
  a.wb[(size_t)b * K + k] = vb;
}

template <bool STAGE>
__global__ __launch_bounds__(kNaNT) void num_arc_count_kernel(const NumArcArgs c) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ int s_max;
  float* const strow = reinterpret_cast<float*>(smem_raw);                     // STAGE: [H] log occupancy of every state at frame t
  const NumArgs& a = c.n;
  const int tid = threadIdx.x, b = blockIdx.y;
  const int L = seq_len(a.lengths, b, a.T);
  const int H = a.H, K = a.K, T = a.T;
  const int t0 = blockIdx.x * kNumArcFrames;
  if (t0 >= L) return;                                                         // (the reduction reads the runs of live frames only)
  const int t1 = min(t0 + kNumArcFrames, L);
  const double logp = a.logp_ws[b];
  if (!(logp - logp == 0.0)) return;                                           // no usable result: the reduction writes zeros
  const size_t g = (size_t)b * a.graph_stride;
  const int32_t* ft = a.fwd_trans + g * K * 3;
  const int Kused = used_arcs(a.fwd_idx + g * H * 2, H, K, &s_max, tid);
  const double* aws = a.alpha_ws + (size_t)b * (T + 1) * H;
  const double* bws = a.beta_ws + (size_t)b * (T + 1) * H;
  const float* fseq = a.frac_ws + (size_t)b * T * K;
  double* const prow = c.partial + ((size_t)b * c.nrun + blockIdx.x) * K;
  if constexpr (STAGE) {
    double acc[kNaReg];
    int src[kNaReg];
#pragma unroll
    for (int i = 0; i < kNaReg; i++) {
      const int k = tid + i * kNaNT;
      acc[i] = 0.0;
      src[i] = k < Kused ? ft[(size_t)3 * k] : 0;
    }
    bool first = true;
    for (int t = t0; t < t1; t++) {
      const double* ar = aws + (size_t)t * H;
      const double* br = bws + (size_t)t * H;
      for (int h = tid; h < H; h += kNaNT) strow[h] = (float)(ar[h] + br[h] - logp);
      __syncthreads();
      const float* frow = fseq + (size_t)t * K;
#pragma unroll
      for (int i = 0; i < kNaReg; i++) {
        const int k = tid + i * kNaNT;
        if (k < Kused) {
          const float st = strow[src[i]];
          const float v = st == -INFINITY ? 0.f : na_exp(st + frow[k]);
          acc[i] += (double)v;
        }
      }
      for (int k = tid + kNaReg * kNaNT; k < Kused; k += kNaNT) {
        const float st = strow[ft[(size_t)3 * k]];
        const float v = st == -INFINITY ? 0.f : na_exp(st + frow[k]);
        prow[k] = first ? (double)v : prow[k] + (double)v;                     // the arc's one owner
      }
      first = false;
      __syncthreads();                                                         // (the row is free for the next frame)
    }
#pragma unroll
    for (int i = 0; i < kNaReg; i++) { const int k = tid + i * kNaNT; if (k < Kused) prow[k] = acc[i]; }
  } else {
    for (int k = tid; k < Kused; k += kNaNT) {
      const size_t s = (size_t)ft[(size_t)3 * k];
      double sum = 0.0;
      for (int t = t0; t < t1; t++) {
        const float st = (float)(aws[(size_t)t * H + s] + bws[(size_t)t * H + s] - logp);
        const float v = st == -INFINITY ? 0.f : na_exp(st + fseq[(size_t)t * K + k]);
        sum += (double)v;
      }
      prow[k] = sum;
    }
  }
  for (int k = Kused + tid; k < K; k += kNaNT) prow[k] = 0.0;                   // padding arcs: exact zeros
}

__global__ __launch_bounds__(kNaNT) void num_arc_reduce_kernel(const NumArcArgs c) {
  const NumArgs& a = c.n;
  const int b = blockIdx.y, K = a.K;
  const int k = blockIdx.x * kNaNT + threadIdx.x;
  const double logp = a.logp_ws[b];
  if (blockIdx.x == 0 && threadIdx.x == 0) c.objf[b] = logp;
  if (k >= K) return;
  double s = 0.0;
  if (logp - logp == 0.0) {
    const int runs = (seq_len(a.lengths, b, a.T) + kNumArcFrames - 1) / kNumArcFrames;
    const double* p = c.partial + (size_t)b * c.nrun * K + k;
    for (int j = 0; j < runs; j++) s += p[(size_t)j * K];
  }
  c.counts[(size_t)b * K + k] = s;
}

}  // namespace

hipError_t launch_num_arc_weights(const NumArcWeightArgs& w, hipStream_t st) {
  hipLaunchKernelGGL(num_arc_weight_kernel, dim3((w.K + kNaNT - 1) / kNaNT, w.B), dim3(kNaNT), 0, st, w);
  return hipGetLastError();
}

bool num_arc_count_staged(int H, bool gather) { return !gather && 4 * (size_t)H <= kNaStageBudget; }

hipError_t launch_num_arc_counts(const NumArcArgs& c, bool gather, hipStream_t st) {
  const dim3 grid(c.nrun, c.n.B);
  if (num_arc_count_staged(c.n.H, gather))
    hipLaunchKernelGGL(num_arc_count_kernel<true>, grid, dim3(kNaNT), 4 * (size_t)c.n.H, st, c);
  else
    hipLaunchKernelGGL(num_arc_count_kernel<false>, grid, dim3(kNaNT), 0, st, c);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(num_arc_reduce_kernel, dim3((c.n.K + kNaNT - 1) / kNaNT, c.n.B), dim3(kNaNT), 0, st, c);
  return hipGetLastError();
}

}  // namespace pychain_hip
