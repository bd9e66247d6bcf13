// xent.hip - the numerator posteriors of a call as cross-entropy targets of a second network output z
// (include/pychain_hip.h: pychain_hip_xent):
//   objective(b,t) = sum_d gamma(t,d) z(t,d) - s(t) logsumexp_d z(t,.),   d / dz = gamma(t,d) - s(t) softmax(z(t,.))_d
// One workgroup per frame.  The row of z is read ONCE (16-byte loads, 8-byte ones of 2-byte rows) into an fp32 row in LDS,
// where it stays between the two reductions and the store; gamma comes from the frame's compact occupancy row (at most K
// words, scattered to the pdf-ids of upd_ws through that LDS row) or, for numerator graphs on the general kernels, from a
// dense fp32 row; the gradient row is written ONCE, in z's type, scale multiplied in, rounded at the store.  Memory-bound:
// (sizeof z + sizeof dz) D bytes per live frame against ~6 D flops and 2 D transcendentals.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <utility>

#include "device_utils.h"
#include "xent.h"

namespace pychain_hip {
namespace {

constexpr int kXnNT = 256;
constexpr size_t kXnMaxLdsRow = 96 * 1024;      // rows beyond: re-read from global memory (dense gamma only)

template <int ZH>
__device__ __forceinline__ void z_load4(const void* z, size_t e, float (&v)[4]) {
  if constexpr (ZH == kXF32) {
    const float4 q = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(z) + e);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    const uint2 q = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(z) + e);
    half2_to_f32(q.x, ZH == kXBf16, v[0], v[1]);
    half2_to_f32(q.y, ZH == kXBf16, v[2], v[3]);
  }
}
template <int ZH>
__device__ __forceinline__ float z_load1(const void* z, size_t e) {
  if constexpr (ZH == kXF32) return reinterpret_cast<const float*>(z)[e];
  else return half_bits_to_f32(reinterpret_cast<const uint16_t*>(z)[e], ZH == kXBf16);
}
template <int ZH>
__device__ __forceinline__ void z_store4(void* g, size_t e, float v0, float v1, float v2, float v3) {
  if constexpr (ZH == kXF32) {
    *reinterpret_cast<float4*>(reinterpret_cast<float*>(g) + e) = make_float4(v0, v1, v2, v3);
  } else {
    uint2 q;
    q.x = pack_half2(v0, v1, ZH == kXBf16); q.y = pack_half2(v2, v3, ZH == kXBf16);
    *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(g) + e) = q;
  }
}
template <int ZH>
__device__ __forceinline__ void z_store1(void* g, size_t e, float v) {
  if constexpr (ZH == kXF32) reinterpret_cast<float*>(g)[e] = v;
  else reinterpret_cast<uint16_t*>(g)[e] = (uint16_t)f32_to_half_bits(v, ZH == kXBf16);
}

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

// ZH: z's element type; VEC: rows of a multiple of four elements (vector loads and stores); GRAD: the gradient row is stored;
// DENSE: gamma from a dense fp32 row instead of the compact one; INLDS: the row fits LDS (else DENSE && !VEC: every pass reads z
// again - rows of more than 24 576 pdfs, which only the general numerator kernels take)
template <int ZH, bool VEC, bool GRAD, bool DENSE, bool INLDS>
__global__ __launch_bounds__(kXnNT) void xent_row_kernel(const XentArgs a) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ float red[3][4];
  const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y, D = a.D, T = a.T;
  const int L = seq_len(a.lengths, b, T);
  const size_t fr = (size_t)b * T + t, row = fr * D;
  const double logp = a.logp[b];
  // a sequence without an admissible path (logP = -inf, or NaN) has gamma = 0: no objective, zero rows
  if (!(t < L && logp - logp == 0.0)) {
    if constexpr (GRAD) {
      if constexpr (VEC) { for (int e = tid * 4; e < D; e += 4 * kXnNT) z_store4<ZH>(a.grad, row + e, 0.f, 0.f, 0.f, 0.f); }
      else { for (int e = tid; e < D; e += kXnNT) z_store1<ZH>(a.grad, row + e, 0.f); }
    }
    if (tid == 0) a.frame_objf[fr] = 0.0;
    return;
  }
  // 1. the row, once: global -> fp32 in LDS, and its maximum (fmaxf passes a NaN by: the sum below meets it)
  float m = -INFINITY;
  if constexpr (VEC) {
    for (int e = tid * 4; e < D; e += 4 * kXnNT) {
      float v[4];
      z_load4<ZH>(a.z, row + e, v);
      *reinterpret_cast<float4*>(srow + e) = make_float4(v[0], v[1], v[2], v[3]);
      m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
  } else {
    for (int e = tid; e < D; e += kXnNT) {
      const float v = z_load1<ZH>(a.z, row + e);
      if constexpr (INLDS) srow[e] = v;
      m = fmaxf(m, v);
    }
  }
  m = block_max(m, red[0]);                          // (its barriers: the LDS row is complete)
  auto zv = [&](int e) -> float { if constexpr (INLDS) return srow[e]; else return z_load1<ZH>(a.z, row + e); };
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
  const int U = DENSE ? 0 : min(a.ucount[b], a.K);
  const float* crow = DENSE ? nullptr : a.rows + fr * a.K;
  const int32_t* upd = DENSE ? nullptr : a.upd + (size_t)b * a.K;
  if constexpr (!DENSE) {
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
  if constexpr (!DENSE) {
    for (int e = e0; e < D; e += estep) {
#pragma unroll
      for (int i = 0; i < ew; i++) srow[e + i] = -(s * expf(srow[e + i] - lse));
    }
    __syncthreads();
    for (int u = tid; u < U; u += kXnNT) {           // (the distinct pdfs of the sequence: one thread per word)
      const float g = crow[u];
      const int n = upd[u];
      if (g != 0.f && (unsigned)n < (unsigned)D) srow[n] += g;
    }
    __syncthreads();
  }
  for (int e = e0; e < D; e += estep) {
    float o[4];
#pragma unroll
    for (int i = 0; i < ew; i++) {
      if constexpr (DENSE) o[i] = sc * fmaf(-s, expf(zv(e + i) - lse), a.dense[row + e + i]);
      else o[i] = sc * srow[e + i];
    }
    if constexpr (VEC) z_store4<ZH>(a.grad, row + e, o[0], o[1], o[2], o[3]);
    else z_store1<ZH>(a.grad, row + e, o[0]);
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

__global__ __launch_bounds__(kXnNT) void xent_totals_kernel(const float* objf, int B, float loss_scale, const float* norm_dev, float coef,
                                                           float* xent_totals, float* totals) {
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
    }
  }
}

template <int ZH, bool VEC, bool GRAD, bool DENSE, bool INLDS>
hipError_t launch_rows_as(const XentArgs& a, size_t lds, hipStream_t st) {
  auto k = xent_row_kernel<ZH, VEC, GRAD, DENSE, INLDS>;
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
    if constexpr (!VEC) return launch_rows_as<ZH, false, GRAD, true, false>(a, 0, st);
    else return hipErrorInvalidValue;
  }
  return a.dense ? launch_rows_as<ZH, VEC, GRAD, true, true>(a, lds, st) : launch_rows_as<ZH, VEC, GRAD, false, true>(a, lds, st);
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
  if (!inlds && !a.dense) { *why = "a row of the cross-entropy output does not fit LDS beside compact occupancy rows"; return hipErrorInvalidValue; }
  const bool vec = inlds && a.D % 4 == 0;
  const size_t lds = inlds ? row_bytes : 0;
  hipError_t e = a.z_half == kXF32 ? launch_rows_z<kXF32>(a, lds, vec, inlds, st)
               : a.z_half == kXBf16 ? launch_rows_z<kXBf16>(a, lds, vec, inlds, st) : launch_rows_z<kXF16>(a, lds, vec, inlds, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(xent_seq_sum_kernel, dim3(a.B), dim3(kXnNT), 0, st, a.frame_objf, a.lengths, a.T, a.objf);
  return hipGetLastError();
}

hipError_t launch_xent_totals(const float* objf, int B, float loss_scale, const float* norm_dev, float coef, float* xent_totals,
                              float* totals, hipStream_t st) {
  hipLaunchKernelGGL(xent_totals_kernel, dim3(1), dim3(kXnNT), 0, st, objf, B, loss_scale, norm_dev, coef, xent_totals, totals);
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
