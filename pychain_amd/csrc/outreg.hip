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
#include <cstring>

#include "../../include/pychain_hip.h"
#include "common.h"
#include "row_access.h"

namespace pychain_hip {

enum { kRegNoGrad = 0, kRegAccum = 1, kRegLinear = 2 };

// (used by this file alone; outside the unnamed namespace because the kernels' symbols carry its name)
struct OutRegArgs {
  const void* x;             // [B,T,D] raw, x_half: 0 fp32, kXBf16 / kXF16 (device_utils.h): 2-byte rows are read as they are
  int x_half;
  void* grad;                // [B,T,D] in x's type, or nullptr (mode kRegNoGrad)
  int mode;
  float l2, oor, limit;
  float scale;               // s = scale [* *scale_dev] [/ *norm_dev]
  const float* scale_dev;
  const float* norm_dev;
  const int64_t* lengths;    // [B]
  double* frame_pairs;       // [B,T,2] scratch: {sum x^2, sum e^2} of every live frame
  double* seq_pairs;         // [B,2] scratch: the unrounded per-sequence sums
  float* per_seq;            // [B,2] out
  int B, T, D;
};

namespace {

constexpr int kRgNT = 256;                          // four waves
constexpr int kRgRows = 2;                          // frames in flight per wave
constexpr int kRgChunk = (kRgNT / 64) * kRgRows;    // frames of one work item

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

// XH: x's (and the gradient's) element type; VW: elements per load and store (row_access.h: fp32 4 / 1, 2-byte 8 / 4 / 1, the
// widest that divides D); MODE: kReg*
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
        row_load<XH, VW>(a.x, row0 + e, xa);
        row_load<XH, VW>(a.x, row1 + e, xb);
        if constexpr (MODE == kRegAccum) {
          row_load<XH, VW>(a.grad, row0 + e, ga);
          row_load<XH, VW>(a.grad, row1 + e, gb);
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
          row_store<XH, VW>(a.grad, row0 + e, ga);
          if (two) row_store<XH, VW>(a.grad, row1 + e, gb);
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
          for (int e = lane * VW; e < D; e += 64 * VW) row_store<XH, VW>(a.grad, row + e, z);
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
// the streaming pass over the live rows, then the per-sequence sums of the frame pairs in fp64, fixed order
hipError_t launch_outreg_rows(const OutRegArgs& a, hipStream_t st) {
  const int nchunk = (a.T + kRgChunk - 1) / kRgChunk;
  const size_t items = (size_t)a.B * nchunk;
  if (items > (size_t)INT_MAX) return hipErrorInvalidValue;
  if ((a.mode == kRegNoGrad) != (a.grad == nullptr)) return hipErrorInvalidValue;
  const int nitems = (int)items, grid = nitems < kRowPassMaxGrid ? nitems : kRowPassMaxGrid;
  const hipError_t e = row_width_dispatch(a.x_half, a.D, [&](auto xh, auto vw) {
    return launch_rows_as<decltype(xh)::value, decltype(vw)::value>(a, grid, nchunk, nitems, st);
  });
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(outreg_seq_sum_kernel, dim3(a.B), dim3(kRgNT), 0, st, a.frame_pairs, a.lengths, a.T, a.seq_pairs, a.per_seq);
  return hipGetLastError();
}

// reg_totals[0] = loss_scale * (0.5 l2 S2 + oor SO) [/ *norm_dev], [1] = S2, [2] = SO; totals (or nullptr): [0] and [4] += that
hipError_t launch_outreg_totals(const double* seq_pairs, int B, float l2, float oor, float loss_scale, const float* norm_dev,
                                float* reg_totals, float* totals, hipStream_t st) {
  hipLaunchKernelGGL(outreg_totals_kernel, dim3(1), dim3(1), 0, st, seq_pairs, B, l2, oor, loss_scale, norm_dev, reg_totals, totals);
  return hipGetLastError();
}

size_t outreg_workspace_bytes(int B, int T) { return 16 * (size_t)B * T + 16 * (size_t)B; }

}  // namespace
}  // namespace pychain_hip

using namespace pychain_hip;

// ---- the entry points (include/pychain_hip.h) -----------------------------------------------------------------------------------
extern "C" size_t pychain_hip_output_reg_workspace_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  return align256(outreg_workspace_bytes(B, T)) + 256;
}

extern "C" int pychain_hip_output_reg(
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    float l2, float oor, float limit, int grad_mode, void* grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    float* reg_per_seq, float loss_scale, float* reg_totals, float* totals,
    void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "output_reg";
  if (nnet_output_dtype < PYCHAIN_HIP_F32 || nnet_output_dtype > PYCHAIN_HIP_F16)
    return fail(PYCHAIN_HIP_EINVAL, "%s: unknown nnet_output_dtype %d", who, nnet_output_dtype);
  if (!nnet_output || !seq_lengths || !reg_per_seq || !workspace) return fail(PYCHAIN_HIP_EINVAL, "%s: null pointer argument", who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (!(l2 >= 0.f) || !(oor >= 0.f) || !(limit >= 0.f))
    return fail(PYCHAIN_HIP_EINVAL, "%s: l2, oor and limit must not be negative (got %g, %g, %g)", who, (double)l2, (double)oor, (double)limit);
  if (grad_mode != PYCHAIN_HIP_GRAD_ACCUM && grad_mode != PYCHAIN_HIP_GRAD_LINEAR)
    return fail(PYCHAIN_HIP_EINVAL, "%s: grad_mode must be PYCHAIN_HIP_GRAD_ACCUM or PYCHAIN_HIP_GRAD_LINEAR, got %d", who, grad_mode);
  if (((uintptr_t)nnet_output | (uintptr_t)grad | (uintptr_t)workspace) & 15)
    return fail(PYCHAIN_HIP_EINVAL, "%s: nnet_output, grad and workspace must be 16-byte aligned", who);
  const size_t need = pychain_hip_output_reg_workspace_bytes(B, T);
  if (workspace_bytes < need) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  OutRegArgs a;
  memset(&a, 0, sizeof(a));
  a.x = nnet_output; a.x_half = nnet_output_dtype; a.grad = grad;
  a.mode = !grad ? kRegNoGrad : (grad_mode == PYCHAIN_HIP_GRAD_ACCUM ? kRegAccum : kRegLinear);
  a.l2 = l2; a.oor = oor; a.limit = limit; a.scale = grad_scale; a.scale_dev = grad_scale_dev; a.norm_dev = loss_norm_dev;
  a.lengths = seq_lengths; a.frame_pairs = (double*)ws; a.seq_pairs = (double*)(ws + 16 * (size_t)B * T); a.per_seq = reg_per_seq;
  a.B = B; a.T = T; a.D = D;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_outreg_rows(a, st);
  if (e == hipSuccess && (reg_totals || totals)) e = launch_outreg_totals(a.seq_pairs, B, l2, oor, loss_scale, loss_norm_dev, reg_totals, totals, st);
  if (e != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "%s: %s", who, hipGetErrorString(e));
  return PYCHAIN_HIP_OK;
}
