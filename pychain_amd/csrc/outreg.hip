// outreg.hip - the two element-wise regularisers of the chain objective over the network output x [B,T,D] itself
// (include/pychain_hip.h: pychain_hip_output_reg): output L2 and the out-of-range penalty,
//   R2_b = sum_{t<L_b} sum_d x^2,   RO_b = sum_{t<L_b} sum_d e(x)^2,   e(x) = max(|x| - limit, 0) on the RAW x,
//   term(x) = l2 x + 2 oor sign(x) e(x).
// One streaming pass over the LIVE rows: x is read once (16-byte loads; 2-byte rows as they are, 16- or 8-byte loads), the
// stored gradient row once (ACCUM), the gradient row is written once in x's type.  Rows t >= L_b are never read; LINEAR
// writes zeros there, ACCUM and the objective-only form do not touch them.  Memory-bound: at most 3 sizeof(x) D bytes per
// live frame against ~16 D flops, so the fp64 of the sums is free.
//
// A capped grid of four-wave workgroups strides over (sequence, chunk of 8 frames) items; every wave of an item owns TWO
// frames at a time and keeps a vector of each (and of each stored gradient row) in flight, its row loop unrolled twice.
//
// THE OPERATION SEQUENCE (the tests count these roundings).  x is the fp32 value of the element (2-byte elements widen
// exactly).  Sums, fp64 from the first add:
//     xd = (double)x                          exact
//     r2 = fma(xd, xd, r2)                    x^2 is exact in fp64: one rounding, the add
//     ad = |xd| - (double)limit               exact
//     ed = ad if !(ad <= 0) else 0            (a NaN stays a NaN, as torch.clamp keeps it)
//     ro = fma(ed, ed, ro)                    one rounding
// per lane over its elements of the frame in ascending order, then over the wave by the xor butterfly 32, 16, .. 1 (every
// lane ends with the same bits), lane 0 stores the frame's {r2, ro}; outreg_seq_sum_kernel adds the frames of a sequence
// (thread by thread in ascending t, butterfly, the four waves pairwise) and rounds to fp32 ONCE; outreg_totals_kernel adds the
// unrounded per-sequence sums in ascending b on one thread.  No atomics: the same call gives the same bits.
// Gradient term, plain fp32, contraction off - at most 7 roundings:
//     s    = scale [* *scale_dev] [/ *norm_dev]      0, 1 or 2 roundings
//     a    = l2 * x                                  1
//     e    = max(|x| - limit, 0)                     1   (exact for |x| <= 2 limit)
//     u    = fmaf(2 oor, copysign(e, x), a)          1   (2 oor is exact)
//     term = s * u                                   1
//     ACCUM:  g' = g + term                          1   LINEAR: g = term
// and, for 2-byte gradients, the rounding to nearest even at the store.  A 2-BYTE GRADIENT IN ACCUM IS THEREFORE ROUNDED
// TWICE: the fused call stored it rounded to bf16 / fp16, and this pass rounds the sum again (the single-rounding end state -
// the term folded into the store of den_gamma2_kernel - is DESIGN.md §8's lead).
#include <hip/hip_runtime.h>

#include <climits>

#include "device_utils.h"
#include "outreg.h"

namespace pychain_hip {
namespace {

constexpr int kRgNT = 256;                          // four waves
constexpr int kRgRows = 2;                          // frames in flight per wave
constexpr int kRgChunk = (kRgNT / 64) * kRgRows;    // frames of one work item
constexpr int kRgMaxGrid = 2048;                    // 256 CUs x 8 workgroups: the rest is strided over

// VW elements at element offset e: 16 bytes (fp32 x 4, 2-byte x 8), 8 bytes (2-byte x 4) or one element
template <int XH, int VW>
__device__ __forceinline__ void rg_load(const void* p, size_t e, float (&v)[VW]) {
  if constexpr (XH == kXF32) {
    static_assert(VW == 4 || VW == 1, "fp32 rows: float4 or one element");
    if constexpr (VW == 4) {
      const float4 q = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + e);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = reinterpret_cast<const float*>(p)[e];
    }
  } else {
    static_assert(VW == 8 || VW == 4 || VW == 1, "2-byte rows: eight, four or one element");
    constexpr bool BF = XH == kXBf16;
    const uint16_t* h = reinterpret_cast<const uint16_t*>(p) + e;
    if constexpr (VW == 8) {
      const uint4 q = *reinterpret_cast<const uint4*>(h);
      half2_to_f32(q.x, BF, v[0], v[1]); half2_to_f32(q.y, BF, v[2], v[3]);
      half2_to_f32(q.z, BF, v[4], v[5]); half2_to_f32(q.w, BF, v[6], v[7]);
    } else if constexpr (VW == 4) {
      const uint2 q = *reinterpret_cast<const uint2*>(h);
      half2_to_f32(q.x, BF, v[0], v[1]); half2_to_f32(q.y, BF, v[2], v[3]);
    } else {
      v[0] = half_bits_to_f32(*h, BF);
    }
  }
}
template <int XH, int VW>
__device__ __forceinline__ void rg_store(void* p, size_t e, const float (&v)[VW]) {
  if constexpr (XH == kXF32) {
    if constexpr (VW == 4) *reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + e) = make_float4(v[0], v[1], v[2], v[3]);
    else reinterpret_cast<float*>(p)[e] = v[0];
  } else {
    constexpr bool BF = XH == kXBf16;
    uint16_t* h = reinterpret_cast<uint16_t*>(p) + e;
    if constexpr (VW == 8) {
      uint4 q;
      q.x = pack_half2(v[0], v[1], BF); q.y = pack_half2(v[2], v[3], BF);
      q.z = pack_half2(v[4], v[5], BF); q.w = pack_half2(v[6], v[7], BF);
      *reinterpret_cast<uint4*>(h) = q;
    } else if constexpr (VW == 4) {
      uint2 q;
      q.x = pack_half2(v[0], v[1], BF); q.y = pack_half2(v[2], v[3], BF);
      *reinterpret_cast<uint2*>(h) = q;
    } else {
      *h = (uint16_t)f32_to_half_bits(v[0], BF);
    }
  }
}

// the two sums of one element (header: fp64 from the first add)
__device__ __forceinline__ void rg_sums(float x, double limd, double& r2, double& ro) {
  const double xd = (double)x;
  r2 = fma(xd, xd, r2);
  const double ad = fabs(xd) - limd;
  const double ed = !(ad <= 0.0) ? ad : 0.0;
  ro = fma(ed, ed, ro);
}
// s * (l2 x + 2 oor sign(x) e(x)) [+ g]: the fp32 sequence of the header, nothing contracted
template <bool ACCUM>
__device__ __forceinline__ float rg_grad(float x, float g, float l2, float oor2, float lim, float s) {
#pragma clang fp contract(off)
  const float a = l2 * x;
  const float e = fmaxf(fabsf(x) - lim, 0.f);
  const float u = __builtin_fmaf(oor2, copysignf(e, x), a);
  const float term = s * u;
  if constexpr (ACCUM) return g + term;
  else return term;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// XH: x's (and the gradient's) element type; VW: elements per load (1: rows whose base is not aligned); MODE: kReg*
template <int XH, int VW, int MODE>
__global__ __launch_bounds__(kRgNT) void outreg_rows_kernel(const OutRegArgs a, int nchunk, int nitems) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int T = a.T, D = a.D;
  float s = 0.f;
  if constexpr (MODE != kRegNoGrad) {
    s = a.scale_dev ? a.scale * *a.scale_dev : a.scale;
    if (a.norm_dev) s = s / *a.norm_dev;
  }
  const float l2 = a.l2, oor2 = 2.f * a.oor, lim = a.limit;
  const double limd = (double)a.limit;
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int b = item / nchunk, t0 = (item - b * nchunk) * kRgChunk + wave * kRgRows;
    const int L = seq_len(a.lengths, b, T);
    const size_t seq = (size_t)b * T;
    if (t0 < L) {
      // the wave's second frame; where the sequence ends on the first, that one is read again and nothing is stored for it
      const bool two = t0 + 1 < L;
      const size_t row0 = (seq + t0) * D, row1 = two ? row0 + D : row0;
      double r2a = 0.0, roa = 0.0, r2b = 0.0, rob = 0.0;
#pragma unroll 2
      for (int e = lane * VW; e < D; e += 64 * VW) {
        float xa[VW], xb[VW], ga[VW], gb[VW];
        rg_load<XH, VW>(a.x, row0 + e, xa);
        rg_load<XH, VW>(a.x, row1 + e, xb);
        if constexpr (MODE == kRegAccum) {
          rg_load<XH, VW>(a.grad, row0 + e, ga);
          rg_load<XH, VW>(a.grad, row1 + e, gb);
        }
#pragma unroll
        for (int i = 0; i < VW; i++) {
          rg_sums(xa[i], limd, r2a, roa);
          rg_sums(xb[i], limd, r2b, rob);
          if constexpr (MODE != kRegNoGrad) {
            ga[i] = rg_grad<MODE == kRegAccum>(xa[i], MODE == kRegAccum ? ga[i] : 0.f, l2, oor2, lim, s);
            gb[i] = rg_grad<MODE == kRegAccum>(xb[i], MODE == kRegAccum ? gb[i] : 0.f, l2, oor2, lim, s);
          }
        }
        if constexpr (MODE != kRegNoGrad) {
          rg_store<XH, VW>(a.grad, row0 + e, ga);
          if (two) rg_store<XH, VW>(a.grad, row1 + e, gb);
        }
      }
      r2a = wave_sum_f64(r2a); roa = wave_sum_f64(roa);
      r2b = wave_sum_f64(r2b); rob = wave_sum_f64(rob);
      if (lane == 0) {
        double* fp = a.frame_pairs + (seq + t0) * 2;
        fp[0] = r2a; fp[1] = roa;
        if (two) { fp[2] = r2b; fp[3] = rob; }
      }
    }
    if constexpr (MODE == kRegLinear) {              // zeros beyond the length (never read: only written)
      float z[VW];
#pragma unroll
      for (int i = 0; i < VW; i++) z[i] = 0.f;
      for (int r = 0; r < kRgRows; r++) {
        const int t = t0 + r;
        if (t >= L && t < T) {
          const size_t row = (seq + t) * D;
          for (int e = lane * VW; e < D; e += 64 * VW) rg_store<XH, VW>(a.grad, row + e, z);
        }
      }
    }
  }
}

// {R2_b, RO_b} = the sums of the live frames' pairs: fp64, fixed order (the pattern of xent_seq_sum_kernel), rounded once
__global__ __launch_bounds__(kRgNT) void outreg_seq_sum_kernel(const double* frame_pairs, const int64_t* lengths, int T, double* seq_pairs,
                                                              float* per_seq) {
  __shared__ double part[2][4];
  const int b = blockIdx.x, L = seq_len(lengths, b, T);
  const double2* fp = reinterpret_cast<const double2*>(frame_pairs) + (size_t)b * T;
  double a2 = 0.0, ao = 0.0;
  for (int t = threadIdx.x; t < L; t += kRgNT) { const double2 q = fp[t]; a2 += q.x; ao += q.y; }
  a2 = wave_sum_f64(a2); ao = wave_sum_f64(ao);
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = a2; part[1][threadIdx.x >> 6] = ao; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s2 = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
    const double so = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
    seq_pairs[2 * b] = s2; seq_pairs[2 * b + 1] = so;
    per_seq[2 * b] = (float)s2; per_seq[2 * b + 1] = (float)so;
  }
}

// one thread, in stream order behind whatever wrote `totals` (a coefficient of zero leaves its sum out of the loss altogether)
__global__ void outreg_totals_kernel(const double* seq_pairs, int B, float l2, float oor, float loss_scale, const float* norm_dev,
                                     float* reg_totals, float* totals) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s2 = 0.0, so = 0.0;
  for (int b = 0; b < B; b++) { s2 += seq_pairs[2 * b]; so += seq_pairs[2 * b + 1]; }
  double v = (double)loss_scale * ((l2 != 0.f ? 0.5 * (double)l2 * s2 : 0.0) + (oor != 0.f ? (double)oor * so : 0.0));
  if (norm_dev) v /= (double)*norm_dev;
  if (reg_totals) { reg_totals[0] = (float)v; reg_totals[1] = (float)s2; reg_totals[2] = (float)so; }
  if (totals) {
    const float full = (float)((double)totals[0] + v);
    totals[0] = full; totals[4] = full;
  }
}

template <int XH, int VW>
hipError_t launch_rows_as(const OutRegArgs& a, int grid, int nchunk, int nitems, hipStream_t st) {
  if (a.mode == kRegAccum) hipLaunchKernelGGL((outreg_rows_kernel<XH, VW, kRegAccum>), dim3(grid), dim3(kRgNT), 0, st, a, nchunk, nitems);
  else if (a.mode == kRegLinear) hipLaunchKernelGGL((outreg_rows_kernel<XH, VW, kRegLinear>), dim3(grid), dim3(kRgNT), 0, st, a, nchunk, nitems);
  else hipLaunchKernelGGL((outreg_rows_kernel<XH, VW, kRegNoGrad>), dim3(grid), dim3(kRgNT), 0, st, a, nchunk, nitems);
  return hipGetLastError();
}
template <int XH>
hipError_t launch_rows_half(const OutRegArgs& a, int grid, int nchunk, int nitems, hipStream_t st) {
  if (a.D % 8 == 0) return launch_rows_as<XH, 8>(a, grid, nchunk, nitems, st);
  if (a.D % 4 == 0) return launch_rows_as<XH, 4>(a, grid, nchunk, nitems, st);
  return launch_rows_as<XH, 1>(a, grid, nchunk, nitems, st);
}

}  // namespace

size_t outreg_workspace_bytes(int B, int T) { return 16 * (size_t)B * T + 16 * (size_t)B; }

hipError_t launch_outreg_rows(const OutRegArgs& a, hipStream_t st) {
  const int nchunk = (a.T + kRgChunk - 1) / kRgChunk;
  const size_t items = (size_t)a.B * nchunk;
  if (items > (size_t)INT_MAX) return hipErrorInvalidValue;
  if ((a.mode == kRegNoGrad) != (a.grad == nullptr)) return hipErrorInvalidValue;
  const int nitems = (int)items, grid = nitems < kRgMaxGrid ? nitems : kRgMaxGrid;
  hipError_t e;
  if (a.x_half == kXF32) e = a.D % 4 == 0 ? launch_rows_as<kXF32, 4>(a, grid, nchunk, nitems, st) : launch_rows_as<kXF32, 1>(a, grid, nchunk, nitems, st);
  else if (a.x_half == kXBf16) e = launch_rows_half<kXBf16>(a, grid, nchunk, nitems, st);
  else e = launch_rows_half<kXF16>(a, grid, nchunk, nitems, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(outreg_seq_sum_kernel, dim3(a.B), dim3(kRgNT), 0, st, a.frame_pairs, a.lengths, a.T, a.seq_pairs, a.per_seq);
  return hipGetLastError();
}

hipError_t launch_outreg_totals(const double* seq_pairs, int B, float l2, float oor, float loss_scale, const float* norm_dev,
                                float* reg_totals, float* totals, hipStream_t st) {
  hipLaunchKernelGGL(outreg_totals_kernel, dim3(1), dim3(1), 0, st, seq_pairs, B, l2, oor, loss_scale, norm_dev, reg_totals, totals);
  return hipGetLastError();
}

}  // namespace pychain_hip
