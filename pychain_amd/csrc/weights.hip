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
#include <cstring>

#include "../../include/pychain_hip.h"
#include "common.h"
#include "row_access.h"

namespace pychain_hip {

// (both used by this file alone; outside the unnamed namespace because the kernels' symbols carry their names)
struct WeightRowsArgs {
  void* grad;                // [B,T,D], dtype: 0 fp32, kXBf16 / kXF16 (device_utils.h)
  int dtype;
  const int64_t* lengths;    // [B]
  const float* u;            // [B] or nullptr (= 1)
  const float* f;            // [B,T] or nullptr (= 1)
  int B, T, D;
};

struct WeightSumsArgs {
  const int64_t* lengths;    // [B]
  const float* u;            // [B] or nullptr (= 1)
  const float* den;          // [B]
  const float* num;          // [B]
  const float* xent;         // [B] or nullptr
  const float* reg;          // [B][2] = {R2_b, RO_b} or nullptr
  float xent_coef, l2, oor, loss_scale;
  const float* norm_dev;     // or nullptr
  float* totals;             // [PYCHAIN_HIP_TOTALS] or nullptr
  float* weighted;           // [5] or nullptr
  int B, T;
};

namespace {

constexpr int kWtNT = 256;                 // four waves
constexpr int kWtItem = 32768;             // elements of one work item, about
constexpr int kWtFlatBelow = 64;           // rows narrower than a wave: the flat form

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
    row_load<XH, VW>(g, e, v);
#pragma unroll
    for (int i = 0; i < VW; i++) v[i] = v[i] * w;
  }
  row_store<XH, VW>(g, e, v);
}

// rows form: `chunk` frames per item (a multiple of 4), wave `k` of the item takes its frames k, k + 4, ...
// (both forms: VW = row_access.h's widths - fp32 4 / 1, 2-byte 8 / 4 / 1, the widest that divides D)
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
    const int grid = items < (size_t)kRowPassMaxGrid ? (int)items : kRowPassMaxGrid;
    hipLaunchKernelGGL((weight_rows_kernel<XH, VW>), dim3(grid), dim3(kWtNT), 0, st, a, chunk, nchunk, (int)items);
  } else {
    const size_t live = (size_t)a.T * a.D;
    if (live > (size_t)INT_MAX - kWtItem) return hipErrorInvalidValue;
    const int nspan = (int)((live + kWtItem - 1) / kWtItem);
    const size_t items = (size_t)a.B * nspan;
    if (items > (size_t)INT_MAX) return hipErrorInvalidValue;
    const int grid = items < (size_t)kRowPassMaxGrid ? (int)items : kRowPassMaxGrid;
    hipLaunchKernelGGL((weight_flat_kernel<XH, VW>), dim3(grid), dim3(kWtNT), 0, st, a, kWtItem, nspan, (int)items);
  }
  return hipGetLastError();
}
// the streaming pass over the live rows whose weight is neither 1 (not touched) nor 0 (zeros stored, nothing loaded)
hipError_t launch_weight_rows(const WeightRowsArgs& a, hipStream_t st) {
  if (!a.grad || !a.lengths || (!a.u && !a.f) || a.B <= 0 || a.T <= 0 || a.D <= 0) return hipErrorInvalidValue;
  return row_width_dispatch(a.dtype, a.D, [&](auto xh, auto vw) { return launch_as<decltype(xh)::value, decltype(vw)::value>(a, st); });
}

// one thread, fp64, ascending b, in stream order behind whatever wrote `totals` and the per-sequence arrays
hipError_t launch_weight_sums(const WeightSumsArgs& s, hipStream_t st) {
  hipLaunchKernelGGL(weight_sums_kernel, dim3(1), dim3(1), 0, st, s);
  return hipGetLastError();
}

}  // namespace
}  // namespace pychain_hip

using namespace pychain_hip;

// ---- the entry point (include/pychain_hip.h) ------------------------------------------------------------------------------------
extern "C" int pychain_hip_weight_rows(
    void* grad, int grad_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const float* utt_weights, const float* deriv_weights,
    const float* den_objf_per_seq, const float* num_objf_per_seq, const float* xent_objf_per_seq, float xent_coef,
    const float* reg_per_seq, float l2, float oor, float loss_scale, const float* loss_norm_dev,
    float* totals, float* weighted, void* stream) {
  const char* who = "weight_rows";
  if (!utt_weights && !deriv_weights) return fail(PYCHAIN_HIP_EINVAL, "%s: neither utt_weights nor deriv_weights", who);
  if (!seq_lengths) return fail(PYCHAIN_HIP_EINVAL, "%s: null seq_lengths", who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (grad && (grad_dtype < PYCHAIN_HIP_F32 || grad_dtype > PYCHAIN_HIP_F16)) return fail(PYCHAIN_HIP_EINVAL, "%s: unknown grad_dtype %d", who, grad_dtype);
  if ((uintptr_t)grad & 15) return fail(PYCHAIN_HIP_EINVAL, "%s: grad must be 16-byte aligned", who);
  const bool sums = totals || weighted;
  if (!grad && !sums) return fail(PYCHAIN_HIP_EINVAL, "%s: nothing to do (no grad, no totals, no weighted)", who);
  if (sums && (!den_objf_per_seq || !num_objf_per_seq)) return fail(PYCHAIN_HIP_EINVAL, "%s: the sums need den_objf_per_seq and num_objf_per_seq", who);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  if (grad) {
    WeightRowsArgs a;
    memset(&a, 0, sizeof(a));
    a.grad = grad; a.dtype = grad_dtype; a.lengths = seq_lengths; a.u = utt_weights; a.f = deriv_weights; a.B = B; a.T = T; a.D = D;
    e = launch_weight_rows(a, st);
  }
  if (e == hipSuccess && sums) {
    WeightSumsArgs s;
    memset(&s, 0, sizeof(s));
    s.lengths = seq_lengths; s.u = utt_weights; s.den = den_objf_per_seq; s.num = num_objf_per_seq; s.xent = xent_objf_per_seq;
    s.reg = reg_per_seq; s.xent_coef = xent_coef; s.l2 = l2; s.oor = oor; s.loss_scale = loss_scale; s.norm_dev = loss_norm_dev;
    s.totals = totals; s.weighted = weighted; s.B = B; s.T = T;
    e = launch_weight_sums(s, st);
  }
  if (e != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "%s: %s", who, hipGetErrorString(e));
  return PYCHAIN_HIP_OK;
}
