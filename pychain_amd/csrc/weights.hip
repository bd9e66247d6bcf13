// weights.hip - utterance weights u [B] and per-frame derivative weights f [B,T] of the chain objective (Kaldi:
// Supervision::weight, NnetChainSupervision::deriv_weights) applied to a gradient the fused call has already written
// (include/pychain_hip.h: pychain_hip_weight_rows).  Per live row (b, t < L_b), w = fl32(u_b * f_bt):
//     w == 1     the row is neither read nor written
//     w == 0     the row is stored as +0 without a load (a NaN in it is gone)
//     else       every element widened to fp32 (exact), multiplied ONCE by w, rounded ONCE (to nearest even) to the
//                gradient's type at the store - one IEEE multiply and one rounding, which the tests hold bit for bit
// Rows t >= L_b are never touched.  The pass moves the bytes of the rows it changes and nothing else: derivative weights
// that are 1 except at chunk edges cost the edge rows.
//
// Two forms, both a capped grid of four-wave workgroups striding over items of AT MOST about kWtItem elements of ONE sequence:
// the launch is never one workgroup per row (B * T idle workgroups at D = 1).  An item does not span sequences, so a narrow
// row makes smaller items - D = 1, T = 1500 is B items of 1500 elements - and in the rows form a row shorter than a wave's
// 64 vectors leaves lanes idle (D = 64 in bf16: 8 of 64); both are small-D cases whose whole gradient is small.
//   rows (D >= 64)  item = (sequence, chunk of frames); a WAVE owns a row at a time, so its weight is wave-uniform (made a
//                   scalar by readfirstlane) and the skip / zero / scale branches do not diverge; 16-byte accesses where
//                   the rows allow (fp32 rows of a multiple of 4 elements, 2-byte rows of a multiple of 8), 8-byte ones for
//                   2-byte rows of a multiple of 4, else element by element; the row loop keeps two vectors in flight
//   flat (D < 64)   item = (sequence, span of elements of its live region); a THREAD owns a vector, which never crosses a
//                   row (D is a multiple of the vector width), and reads its own row's weight
// The weighted sums (fp64, ascending b on one thread, no atomics, rounded once) are a one-thread launch behind the rows.
#include <hip/hip_runtime.h>

#include <climits>

#include "device_utils.h"
#include "weights.h"

namespace pychain_hip {
namespace {

constexpr int kWtNT = 256;                 // four waves
constexpr int kWtItem = 32768;             // elements of one work item, about
constexpr int kWtMaxGrid = 2048;           // 256 CUs x 8 workgroups: the rest is strided over
constexpr int kWtFlatBelow = 64;           // rows narrower than a wave: the flat form

// VW elements at element offset e: 16 bytes (fp32 x 4, 2-byte x 8), 8 bytes (2-byte x 4) or one element
template <int XH, int VW>
__device__ __forceinline__ void wt_load(const void* p, size_t e, float (&v)[VW]) {
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
__device__ __forceinline__ void wt_store(void* p, size_t e, const float (&v)[VW]) {
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

// w(b,t) = fl32(u_b * f_bt), a missing factor is 1
__device__ __forceinline__ float wt_weight(const float* f, float ub, size_t bt) { return f ? ub * f[bt] : ub; }

// one vector at element offset e under the weight w (not 1): zeros without a load, or load - one multiply - store
template <int XH, int VW>
__device__ __forceinline__ void wt_apply(void* g, size_t e, float w) {
  float v[VW];
  if (w == 0.f) {
#pragma unroll
    for (int i = 0; i < VW; i++) v[i] = 0.f;
  } else {
    wt_load<XH, VW>(g, e, v);
#pragma unroll
    for (int i = 0; i < VW; i++) v[i] = v[i] * w;
  }
  wt_store<XH, VW>(g, e, v);
}

// rows form: `chunk` frames per item (a multiple of 4), wave `k` of the item takes its frames k, k + 4, ...
template <int XH, int VW>
__global__ __launch_bounds__(kWtNT) void weight_rows_kernel(const WeightRowsArgs a, int chunk, int nchunk, int nitems) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int T = a.T, D = a.D;
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int b = item / nchunk, t0 = (item - b * nchunk) * chunk;
    const int L = seq_len(a.lengths, b, T);
    const int t1 = t0 + chunk < L ? t0 + chunk : L;
    const float ub = a.u ? a.u[b] : 1.f;
    for (int t = t0 + wave; t < t1; t += kWtNT / 64) {
      const size_t bt = (size_t)b * T + t;
      const float w = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wt_weight(a.f, ub, bt))));
      if (w == 1.f) continue;                                   // (wave-uniform: the row is not touched)
      const size_t row = bt * D;
      if (w == 0.f) {
        for (int e = lane * VW; e < D; e += 64 * VW) wt_apply<XH, VW>(a.grad, row + e, 0.f);
      } else {
#pragma unroll 2
        for (int e = lane * VW; e < D; e += 64 * VW) wt_apply<XH, VW>(a.grad, row + e, w);
      }
    }
  }
}

// flat form: `span` elements per item (a multiple of kWtNT * 8) of the sequence's live region [0, L_b * D)
template <int XH, int VW>
__global__ __launch_bounds__(kWtNT) void weight_flat_kernel(const WeightRowsArgs a, int span, int nspan, int nitems) {
  const int T = a.T, D = a.D;
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int b = item / nspan, e0 = (item - b * nspan) * span;
    const int live = seq_len(a.lengths, b, T) * D;              // (T * D < 64 T fits an int: launch_weight_rows checks)
    const int e1 = e0 + span < live ? e0 + span : live;
    const float ub = a.u ? a.u[b] : 1.f;
    const size_t seq = (size_t)b * T;
    for (int e = e0 + (int)threadIdx.x * VW; e < e1; e += kWtNT * VW) {
      const float w = wt_weight(a.f, ub, seq + e / D);
      if (w != 1.f) wt_apply<XH, VW>(a.grad, seq * D + e, w);
    }
  }
}

// one thread, in stream order behind whatever wrote the per-sequence arrays and `totals`.  An utterance of weight 0 is
// SKIPPED, not multiplied: its objective may be -inf or a NaN and contributes exactly 0.
__global__ void weight_sums_kernel(const WeightSumsArgs s) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double lf = 0.0, sx = 0.0, s2 = 0.0, so = 0.0, sl = 0.0;
  for (int b = 0; b < s.B; b++) {
    const float u = s.u ? s.u[b] : 1.f;
    if (u == 0.f) continue;
    const double ud = (double)u;
    lf += ud * ((double)s.den[b] - (double)s.num[b]);
    if (s.xent) sx += ud * (double)s.xent[b];
    if (s.reg) { s2 += ud * (double)s.reg[2 * b]; so += ud * (double)s.reg[2 * b + 1]; }
    sl += ud * (double)seq_len(s.lengths, b, s.T);
  }
  double v = lf;
  if (s.xent) v += (double)s.xent_coef * sx;
  if (s.reg) v += (s.l2 != 0.f ? 0.5 * (double)s.l2 * s2 : 0.0) + (s.oor != 0.f ? (double)s.oor * so : 0.0);
  v *= (double)s.loss_scale;
  if (s.norm_dev) v /= (double)*s.norm_dev;
  if (s.totals) {
    const float full = (float)v;
    s.totals[0] = full; s.totals[4] = full;
    s.totals[1] = (float)sl; s.totals[3] = (float)lf;
  }
  if (s.weighted) {
    s.weighted[0] = (float)lf; s.weighted[1] = (float)sx; s.weighted[2] = (float)s2; s.weighted[3] = (float)so; s.weighted[4] = (float)sl;
  }
}

template <int XH, int VW>
hipError_t launch_as(const WeightRowsArgs& a, hipStream_t st) {
  if (a.D >= kWtFlatBelow) {
    int chunk = (kWtItem / a.D + 3) & ~3;
    if (chunk < 4) chunk = 4;
    const int nchunk = (a.T + chunk - 1) / chunk;
    const size_t items = (size_t)a.B * nchunk;
    if (items > (size_t)INT_MAX) return hipErrorInvalidValue;
    const int grid = items < (size_t)kWtMaxGrid ? (int)items : kWtMaxGrid;
    hipLaunchKernelGGL((weight_rows_kernel<XH, VW>), dim3(grid), dim3(kWtNT), 0, st, a, chunk, nchunk, (int)items);
  } else {
    const size_t live = (size_t)a.T * a.D;
    if (live > (size_t)INT_MAX - kWtItem) return hipErrorInvalidValue;
    const int nspan = (int)((live + kWtItem - 1) / kWtItem);
    const size_t items = (size_t)a.B * nspan;
    if (items > (size_t)INT_MAX) return hipErrorInvalidValue;
    const int grid = items < (size_t)kWtMaxGrid ? (int)items : kWtMaxGrid;
    hipLaunchKernelGGL((weight_flat_kernel<XH, VW>), dim3(grid), dim3(kWtNT), 0, st, a, kWtItem, nspan, (int)items);
  }
  return hipGetLastError();
}
template <int XH>
hipError_t launch_half(const WeightRowsArgs& a, hipStream_t st) {
  if (a.D % 8 == 0) return launch_as<XH, 8>(a, st);
  if (a.D % 4 == 0) return launch_as<XH, 4>(a, st);
  return launch_as<XH, 1>(a, st);
}

}  // namespace

hipError_t launch_weight_rows(const WeightRowsArgs& a, hipStream_t st) {
  if (!a.grad || !a.lengths || (!a.u && !a.f) || a.B <= 0 || a.T <= 0 || a.D <= 0) return hipErrorInvalidValue;
  if (a.dtype == kXF32) return a.D % 4 == 0 ? launch_as<kXF32, 4>(a, st) : launch_as<kXF32, 1>(a, st);
  if (a.dtype == kXBf16) return launch_half<kXBf16>(a, st);
  return launch_half<kXF16>(a, st);
}

hipError_t launch_weight_sums(const WeightSumsArgs& s, hipStream_t st) {
  hipLaunchKernelGGL(weight_sums_kernel, dim3(1), dim3(1), 0, st, s);
  return hipGetLastError();
}

}  // namespace pychain_hip
