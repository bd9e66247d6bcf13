// xent.hip - the numerator posteriors of a call as cross-entropy targets of a second network output z
// (include/pychain_hip.h: pychain_hip_xent):
//   objective(b,t) = sum_d gamma(t,d) z(t,d) - s(t) logsumexp_d z(t,.),   d / dz = gamma(t,d) - s(t) softmax(z(t,.))_d
// One workgroup per frame.  The row of z is read ONCE (16-byte loads, 8-byte ones of 2-byte rows) into an fp32 row in LDS,
// where it stays between the two reductions and the store; gamma comes from the frame's compact occupancy row (at most K
// words, scattered to the pdf-ids of upd_ws through that LDS row) or, for numerator graphs on the general kernels, from a
// dense fp32 row; the gradient row is written ONCE, in z's type, scale multiplied in, rounded at the store.  Memory-bound:
// (sizeof z + sizeof dz) D bytes per live frame against ~6 D flops and 2 D transcendentals.
// A third source of targets (pychain_hip_xent_targets): sparse entries q(b,t,k) on pdf(b,t,k), K per frame -
// posterior targets from a teacher or a lattice, or an alignment (K = 1).  The same row kernel; a pdf that occurs several times
// in a frame is handled where it occurs first (the later q added to the first in ascending k: the rule of post.hip), so the
// scatter into the LDS row neither races nor needs an atomic; a live frame without a live entry stores zeros and does not read z.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <utility>

#include "../../include/pychain_hip.h"
#include "common.h"
#include "row_access.h"
#include "xent.h"

namespace pychain_hip {
namespace {

constexpr int kXnNT = 256;
constexpr size_t kXnMaxLdsRow = 96 * 1024;      // rows beyond: re-read from global memory (dense gamma and sparse entries)
constexpr int kXnCompact = 0, kXnDense = 1, kXnSparse = 2;      // where the targets of a frame come from

// reductions over the workgroup in a FIXED order (xor butterfly in the wave - every lane ends with the same bits -, then the
// four waves' values pairwise): the same call gives the same bits
__device__ __forceinline__ float block_max(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return r;
}
__device__ __forceinline__ void block_sum3(float& a, float& b, float& c, float (*red)[4]) {
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); c += __shfl_xor(c, o); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; red[2][threadIdx.x >> 6] = c; }
  __syncthreads();
  a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  c = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
  __syncthreads();
}

// sparse entries: the two integer counts of a frame over the workgroup
__device__ __forceinline__ void block_sum2i(int& a, int& b, int (*red)[4]) {
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  __syncthreads();
}
// entry k of a frame's K sparse entries: true where it is live (0 <= pdf < D) and the FIRST of its pdf in the frame; then d = the
// pdf and qd = the fp32 sum of the frame's q with that pdf, in ascending k (nothing to contract: adds only)
__device__ __forceinline__ bool sparse_first(const int32_t* pd, const float* pr, int K, int k, int D, int& d, float& qd) {
  d = pd[k];
  if ((unsigned)d >= (unsigned)D) return false;
  for (int j = 0; j < k; j++)
    if (pd[j] == d) return false;
  qd = pr[k];
  for (int j = k + 1; j < K; j++)
    if (pd[j] == d) qd += pr[j];
  return true;
}

// ZH: z's element type; VEC: rows of a multiple of four elements (row_load<ZH, 4>, row_store4_late; else row_load1, row_store1);
// GRAD: the gradient row is stored;
// SRC: gamma from the compact occupancy row (kXnCompact), from a dense fp32 row (kXnDense) or from sparse entries (kXnSparse);
// INLDS: the row fits LDS (else !VEC and not compact: every pass reads z again - rows of more than 24 576 pdfs, which only the
// general numerator kernels and sparse entries take)
template <int ZH, bool VEC, bool GRAD, int SRC, bool INLDS>
__global__ __launch_bounds__(kXnNT) void xent_row_kernel(const XentArgs a) {
  constexpr bool DENSE = SRC == kXnDense, SPARSE = SRC == kXnSparse;
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ float red[3][4];
  const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y, D = a.D, T = a.T;
  const int L = seq_len(a.lengths, b, T);
  const size_t fr = (size_t)b * T + t, row = fr * D;
  bool live = t < L;
  if constexpr (!SPARSE) {
    // a sequence without an admissible path (logP = -inf, or NaN) has gamma = 0: no objective, zero rows
    const double logp = a.logp[b];
    live = live && logp - logp == 0.0;
  }
  const int32_t* tpd = SPARSE ? a.tpdfs + fr * a.K : nullptr;      // (only formed here: entries of frames t >= L are never read)
  const float* tpr = SPARSE ? a.tprobs + fr * a.K : nullptr;
  if constexpr (SPARSE) {
    if (live) {
      // the frame's live entries and the ones that name a pdf the row does not have; a frame without a live entry stays zero
      // and its row of z is not read
      __shared__ int redi[2][4];
      int nlive = 0, nbad = 0;
      for (int u = tid; u < a.K; u += kXnNT) {
        const int d = tpd[u];
        if (d >= D) nbad++;
        else if (d >= 0) nlive++;
      }
      block_sum2i(nlive, nbad, redi);
      if (tid == 0) a.frame_bad[fr] = nbad;
      live = nlive != 0;
    }
  }
  if (!live) {
    if constexpr (GRAD) {
      if constexpr (VEC) {
        const float zero[4] = {0.f, 0.f, 0.f, 0.f};
        for (int e = tid * 4; e < D; e += 4 * kXnNT) row_store4_late<ZH>(a.grad, row + e, zero);
      }
      else { for (int e = tid; e < D; e += kXnNT) row_store1<ZH>(a.grad, row + e, 0.f); }
    }
    if (tid == 0) a.frame_objf[fr] = 0.0;
    return;
  }
  // 1. the row, once: global -> fp32 in LDS, and its maximum (fmaxf passes a NaN by: the sum below meets it)
  float m = -INFINITY;
  if constexpr (VEC) {
    for (int e = tid * 4; e < D; e += 4 * kXnNT) {
      float v[4];
      row_load<ZH, 4>(a.z, row + e, v);
      *reinterpret_cast<float4*>(srow + e) = make_float4(v[0], v[1], v[2], v[3]);
      m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
  } else {
    for (int e = tid; e < D; e += kXnNT) {
      const float v = row_load1<ZH>(a.z, row + e);
      if constexpr (INLDS) srow[e] = v;
      m = fmaxf(m, v);
    }
  }
  m = block_max(m, red[0]);                          // (its barriers: the LDS row is complete)
  auto zv = [&](int e) -> float { if constexpr (INLDS) return srow[e]; else return row_load1<ZH>(a.z, row + e); };
  // 2. sum of exp(z - max), s = sum of gamma, sum of gamma z - over this thread's elements, then over the workgroup
  float se = 0.f, s = 0.f, dot = 0.f;
  const int e0 = VEC ? tid * 4 : tid, estep = VEC ? 4 * kXnNT : kXnNT, ew = VEC ? 4 : 1;
  for (int e = e0; e < D; e += estep) {
#pragma unroll
    for (int i = 0; i < ew; i++) {
      const float v = zv(e + i);
      se += expf(v - m);
      if constexpr (DENSE) {
        const float g = a.dense[row + e + i];
        if (g != 0.f) { s += g; dot = fmaf(g, v, dot); }
      }
    }
  }
  const int U = SRC != kXnCompact ? 0 : min(a.ucount[b], a.K);
  const float* crow = SRC != kXnCompact ? nullptr : a.rows + fr * a.K;
  const int32_t* upd = SRC != kXnCompact ? nullptr : a.upd + (size_t)b * a.K;
  if constexpr (SPARSE) {
    for (int u = tid; u < a.K; u += kXnNT) {         // (O(K) per entry: K is 1 to 64 in real targets; any K is covered)
      int n;
      float g;
      if (sparse_first(tpd, tpr, a.K, u, D, n, g)) { s += g; dot = fmaf(g, zv(n), dot); }
    }
  }
  if constexpr (SRC == kXnCompact) {
    for (int u = tid; u < U; u += kXnNT) {
      const float g = crow[u];
      const int n = upd[u];
      if (g != 0.f && (unsigned)n < (unsigned)D) { s += g; dot = fmaf(g, srow[n], dot); }
    }
  }
  block_sum3(se, s, dot, red);
  const float lse = m + logf(se);
  if (tid == 0) a.frame_objf[fr] = (double)dot - (double)s * (double)lse;
  if constexpr (!GRAD) return;
  // 3. the gradient row, once: scale * (gamma - s softmax(z)), rounded to z's type at the store
  float sc = a.scale_dev ? a.scale * *a.scale_dev : a.scale;
  if (a.norm_dev) sc = sc / *a.norm_dev;
  constexpr bool SCATTER = !DENSE && INLDS;          // the targets are added into the LDS row ahead of the one store
  if constexpr (SCATTER) {
    for (int e = e0; e < D; e += estep) {
#pragma unroll
      for (int i = 0; i < ew; i++) srow[e + i] = -(s * expf(srow[e + i] - lse));
    }
    __syncthreads();
    if constexpr (SPARSE) {
      for (int u = tid; u < a.K; u += kXnNT) {       // (the distinct pdfs of the frame: one thread per pdf, where it occurs first)
        int n;
        float g;
        if (sparse_first(tpd, tpr, a.K, u, D, n, g)) srow[n] += g;
      }
    } else {
      for (int u = tid; u < U; u += kXnNT) {         // (the distinct pdfs of the sequence: one thread per word)
        const float g = crow[u];
        const int n = upd[u];
        if (g != 0.f && (unsigned)n < (unsigned)D) srow[n] += g;
      }
    }
    __syncthreads();
  }
  for (int e = e0; e < D; e += estep) {
    float o[4];
#pragma unroll
    for (int i = 0; i < ew; i++) {
      if constexpr (DENSE) o[i] = sc * fmaf(-s, expf(zv(e + i) - lse), a.dense[row + e + i]);
      else if constexpr (SCATTER) o[i] = sc * srow[e + i];
      else o[i] = sc * -(s * expf(zv(e + i) - lse));
    }
    if constexpr (VEC) row_store4_late<ZH>(a.grad, row + e, o);
    else row_store1<ZH>(a.grad, row + e, o[0]);
  }
  if constexpr (SPARSE && !INLDS) {
    // the re-reading form: the addressed elements are patched behind the row store (the barrier orders this workgroup's two
    // stores to one address), from z again and not from the rounded gradient - the same operations as the form above
    __syncthreads();
    for (int u = tid; u < a.K; u += kXnNT) {
      int n;
      float g;
      if (sparse_first(tpd, tpr, a.K, u, D, n, g)) row_store1<ZH>(a.grad, row + n, sc * (-(s * expf(zv(n) - lse)) + g));
    }
  }
}

// xent_objf[b] = sum over the live frames of the frame objectives: fp64, fixed order
__global__ __launch_bounds__(kXnNT) void xent_seq_sum_kernel(const double* frame_objf, const int64_t* lengths, int T, float* objf) {
  __shared__ double part[4];
  const int b = blockIdx.x, L = seq_len(lengths, b, T);
  double acc = 0.0;
  for (int t = threadIdx.x; t < L; t += kXnNT) acc += frame_objf[(size_t)b * T + t];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) objf[b] = (float)((part[0] + part[1]) + (part[2] + part[3]));
}

// sparse entries: seq_bad[b] = the live frames' entries that name a pdf the row does not have, then their sum over the batch
__global__ __launch_bounds__(kXnNT) void xent_seq_bad_kernel(const int32_t* frame_bad, const int64_t* lengths, int T, int32_t* seq_bad) {
  __shared__ int part[4];
  const int b = blockIdx.x, L = seq_len(lengths, b, T);
  int acc = 0;
  for (int t = threadIdx.x; t < L; t += kXnNT) acc += frame_bad[(size_t)b * T + t];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) seq_bad[b] = (part[0] + part[1]) + (part[2] + part[3]);
}
__global__ __launch_bounds__(kXnNT) void xent_bad_total_kernel(const int32_t* seq_bad, int B, int32_t* bad_count) {
  __shared__ int part[4];
  int acc = 0;
  for (int i = threadIdx.x; i < B; i += kXnNT) acc += seq_bad[i];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *bad_count = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(kXnNT) void xent_totals_kernel(const float* objf, int B, float loss_scale, const float* norm_dev, float coef,
                                                           float* xent_totals, float* totals, const int32_t* bad_count) {
  __shared__ double part[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < B; i += kXnNT) acc += (double)objf[i];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double S = (part[0] + part[1]) + (part[2] + part[3]);
    double sc = S * (double)loss_scale;
    if (norm_dev) sc /= (double)*norm_dev;
    if (xent_totals) { xent_totals[0] = (float)sc; xent_totals[1] = (float)S; }
    if (totals) {                                    // the full loss: LF-MMI + coef * xent
      const float full = (float)((double)totals[0] + (double)coef * sc);
      totals[0] = full; totals[4] = full;
      if (bad_count) totals[2] = totals[2] + (float)*bad_count;
    }
  }
}

template <int ZH, bool VEC, bool GRAD, int SRC, bool INLDS>
hipError_t launch_rows_as(const XentArgs& a, size_t lds, hipStream_t st) {
  auto k = xent_row_kernel<ZH, VEC, GRAD, SRC, INLDS>;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, dim3(a.T, a.B), dim3(kXnNT), lds, st, a);
  return hipGetLastError();
}
template <int ZH, bool VEC, bool GRAD>
hipError_t launch_rows_g(const XentArgs& a, size_t lds, bool inlds, hipStream_t st) {
  if (!inlds) {
    if constexpr (!VEC) return a.tpdfs ? launch_rows_as<ZH, false, GRAD, kXnSparse, false>(a, 0, st)
                                       : launch_rows_as<ZH, false, GRAD, kXnDense, false>(a, 0, st);
    else return hipErrorInvalidValue;
  }
  if (a.tpdfs) return launch_rows_as<ZH, VEC, GRAD, kXnSparse, true>(a, lds, st);
  return a.dense ? launch_rows_as<ZH, VEC, GRAD, kXnDense, true>(a, lds, st) : launch_rows_as<ZH, VEC, GRAD, kXnCompact, true>(a, lds, st);
}
template <int ZH>
hipError_t launch_rows_z(const XentArgs& a, size_t lds, bool vec, bool inlds, hipStream_t st) {
  if (vec) return a.grad ? launch_rows_g<ZH, true, true>(a, lds, inlds, st) : launch_rows_g<ZH, true, false>(a, lds, inlds, st);
  return a.grad ? launch_rows_g<ZH, false, true>(a, lds, inlds, st) : launch_rows_g<ZH, false, false>(a, lds, inlds, st);
}

}  // namespace

size_t xent_frame_bytes(int B, int T) { return 8 * (size_t)B * T; }

hipError_t launch_xent_rows(const XentArgs& a, hipStream_t st, const char** why) {
  if (a.B > 65535) { *why = "the cross-entropy row kernel takes at most 65535 sequences per call"; return hipErrorInvalidValue; }
  const size_t row_bytes = 4 * (((size_t)a.D + 3) & ~(size_t)3);
  bool inlds = row_bytes <= kXnMaxLdsRow;
  if (!inlds && !a.dense && !a.tpdfs) { *why = "a row of the cross-entropy output does not fit LDS beside compact occupancy rows"; return hipErrorInvalidValue; }
  const bool vec = inlds && a.D % 4 == 0;
  const size_t lds = inlds ? row_bytes : 0;
  hipError_t e = a.z_half == kXF32 ? launch_rows_z<kXF32>(a, lds, vec, inlds, st)
               : a.z_half == kXBf16 ? launch_rows_z<kXBf16>(a, lds, vec, inlds, st) : launch_rows_z<kXF16>(a, lds, vec, inlds, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(xent_seq_sum_kernel, dim3(a.B), dim3(kXnNT), 0, st, a.frame_objf, a.lengths, a.T, a.objf);
  if (a.tpdfs) hipLaunchKernelGGL(xent_seq_bad_kernel, dim3(a.B), dim3(kXnNT), 0, st, a.frame_bad, a.lengths, a.T, a.seq_bad);
  return hipGetLastError();
}

hipError_t launch_xent_bad_total(const int32_t* seq_bad, int B, int32_t* bad_count, hipStream_t st) {
  hipLaunchKernelGGL(xent_bad_total_kernel, dim3(1), dim3(kXnNT), 0, st, seq_bad, B, bad_count);
  return hipGetLastError();
}

hipError_t launch_xent_totals(const float* objf, int B, float loss_scale, const float* norm_dev, float coef, float* xent_totals,
                              float* totals, hipStream_t st, const int32_t* bad_count) {
  hipLaunchKernelGGL(xent_totals_kernel, dim3(1), dim3(kXnNT), 0, st, objf, B, loss_scale, norm_dev, coef, xent_totals, totals, bad_count);
  return hipGetLastError();
}

hipEvent_t xent_join_event(hipStream_t caller) {
  static std::mutex lock;
  static std::map<std::pair<int, hipStream_t>, hipEvent_t> table;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> guard(lock);
  hipEvent_t& ev = table[std::make_pair(dev, caller)];
  if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
  return ev;
}

}  // namespace pychain_hip

using namespace pychain_hip;

// ---- sparse entries as the targets: the entry points (include/pychain_hip.h: pychain_hip_xent_targets) -----------------------
extern "C" size_t pychain_hip_xent_targets_workspace_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  // frame objectives (fp64), the frames' bad entries, the sequences' - and the slack of the alignment to 256 bytes
  return align256(xent_frame_bytes(B, T)) + align256(4 * (size_t)B * T) + align256(4 * (size_t)B) + 256;
}

extern "C" int pychain_hip_xent_targets(
    const void* z, int z_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, void* xent_grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    float* xent_objf_per_seq, int32_t* bad_count, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "xent_targets";
  if (z_dtype < PYCHAIN_HIP_F32 || z_dtype > PYCHAIN_HIP_F16) return fail(PYCHAIN_HIP_EINVAL, "%s: unknown z_dtype %d", who, z_dtype);
  if (!z || !seq_lengths || !target_pdfs || !target_probs || !xent_objf_per_seq || !bad_count || !workspace)
    return fail(PYCHAIN_HIP_EINVAL, "%s: null pointer argument", who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  if (((uintptr_t)z | (uintptr_t)xent_grad | (uintptr_t)workspace) & 15)
    return fail(PYCHAIN_HIP_EINVAL, "%s: z, xent_grad and workspace must be 16-byte aligned", who);
  const size_t need = pychain_hip_xent_targets_workspace_bytes(B, T);
  if (workspace_bytes < need) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  XentArgs a;
  memset(&a, 0, sizeof(a));
  a.z = z; a.z_half = z_dtype; a.grad = xent_grad; a.scale = grad_scale; a.scale_dev = grad_scale_dev; a.norm_dev = loss_norm_dev;
  a.lengths = seq_lengths; a.tpdfs = target_pdfs; a.tprobs = target_probs; a.K = K;
  a.frame_objf = (double*)ws;
  a.frame_bad = (int32_t*)(ws + align256(xent_frame_bytes(B, T)));
  a.seq_bad = (int32_t*)(ws + align256(xent_frame_bytes(B, T)) + align256(4 * (size_t)B * T));
  a.objf = xent_objf_per_seq; a.B = B; a.T = T; a.D = D;
  const char* why = "";
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_xent_rows(a, st, &why);
  if (e == hipSuccess) e = launch_xent_bad_total(a.seq_bad, B, bad_count, st);
  if (e != hipSuccess) return fail(*why ? PYCHAIN_HIP_EUNSUPPORTED : PYCHAIN_HIP_ELAUNCH, "%s: %s", who, *why ? why : hipGetErrorString(e));
  return PYCHAIN_HIP_OK;
}

extern "C" int pychain_hip_xent_add_totals(const float* xent_objf_per_seq, int B, float loss_scale, const float* loss_norm_dev, float loss_coef,
                                           float* xent_totals, float* totals, const int32_t* bad_count, void* stream) {
  const char* who = "xent_add_totals";
  if (!xent_objf_per_seq || (!xent_totals && !totals)) return fail(PYCHAIN_HIP_EINVAL, "%s: null pointer argument", who);
  if (B <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad size B=%d", who, B);
  const hipError_t e = launch_xent_totals(xent_objf_per_seq, B, loss_scale, loss_norm_dev, loss_coef, xent_totals, totals, (hipStream_t)stream,
                                          bad_count);
  if (e != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "%s: %s", who, hipGetErrorString(e));
  return PYCHAIN_HIP_OK;
}
