// boost.hip - the row pass of the boosted denominator (LF-bMMI; include/pychain_hip.h: pychain_hip_boost_rows).
// The boosted objective evaluates the denominator with every path's score lowered by `boost` times its per-frame agreement with
// a reference a(b,t,n) given as sparse per-frame targets (an alignment, or the posterior targets of the numerator):
//   e(b,t,n) = exp(clamp(x(b,t,n), -30, 30)) * exp(-boost * a(b,t,n))           for the live frames t < L_b
// - the margin is applied BEHIND the clamp - and pychain_hip_den_forward_backward(input_is_exp = 1) runs on e as it is: its
// occupancies of those rows are the gradient.  No recursion or occupancy kernel knows about the boost.
//
// boost_rows_kernel.  Memory-bound: one read of x in its own type, one fp32 write of e.  A capped grid of four-wave workgroups
// strides over (sequence, chunk of 8 frames) items; a wave owns TWO rows at a time and keeps a vector of each in flight, its row
// loop unrolled twice (the shape of outreg.hip).  The fp32 side is the wide one and moves 16 bytes per lane: float4 loads of
// fp32 rows, float4 stores of e; a 2-byte row is read 8 bytes per lane, so that a lane's load and its store cover the same four
// elements (as den_exp_rows_kernel reads them).  Rows that are no multiple of 4 elements go element by element.  There is no LDS
// row, so a row may be of any length.
//
// THE FRAME'S ENTRIES ARE APPLIED BEHIND THE DENSE STORE, not merged into it: a frame has K entries against D / 64 elements per
// lane, and a merge would compare every vector of the row with every entry (K compares per vector on every lane) to save K
// four-byte stores that hit lines the wave has just written.  The entries are loaded by the first K lanes (64 at a time) and
// stay in registers; v_readlane hands them round - no LDS, no barrier.  An entry is handled where its pdf occurs first
// (post_frames_kernel's rule): qd = the fp32 sum, in ascending k, of the frame's q_k with that pdf, so a repeated pdf is applied
// once, nothing races and nothing is atomic.  The element is then written BY THE LANE THAT STORED IT in the dense pass
// (lane = (pdf / VW) mod 64): two stores of one thread to one address are ordered, so the dense store needs no wait.
//
// THE OPERATION SEQUENCE, fp32, contraction off:
//     E   = clamp_exp(x, kXExpClamp)            device_utils.h, the mode den_exp_rows_kernel uses: an element no entry addresses
//                                               has that kernel's bits
//     u   = boost * qd                          one rounding
//     F   = v_exp_f32((-u) * fp32(log2 e))      one rounding of the product, then the hardware exp2 (exp_bounded: the same
//                                               two instructions that make E)
//     e   = E * F                               ONE multiply, one rounding
// x of the addressed element is read again (a hit in the line the lane has just read) and E recomputed: the same bits.
// A NaN in a live row becomes exp(-30), as in every kernel that clamps by v_med3_f32; the recursions then never see it, so the
// pass counts it itself: bad_count = the live entries with pdf >= D + the live frames of x that hold a NaN.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "../../include/pychain_hip.h"
#include "boost.h"
#include "common.h"
#include "row_access.h"

namespace pychain_hip {
namespace {

constexpr int kBoNT = 256;                          // four waves
constexpr int kBoRows = 2;                          // rows in flight per wave
constexpr int kBoChunk = (kBoNT / 64) * kBoRows;    // frames of one work item

// exp(-boost * qd): the product rounded, then exp_bounded's two instructions
__device__ __forceinline__ float bo_factor(float boost, float qd) {
#pragma clang fp contract(off)
  const float u = boost * qd;
  return exp_bounded(-u);
}
__device__ __forceinline__ float bo_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float bo_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ int lane_int(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ __forceinline__ float lane_float(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }

// entries k0 + lane of frame f (k0 wave-uniform): (pdf or -1, prob); pdf >= D is counted
__device__ __forceinline__ void bo_entries(const BoostArgs& a, size_t f, int k0, int lane, int& d, float& q, int& bad) {
  d = -1; q = 0.f;
  const int k = k0 + lane;
  if (k < a.K) {
    const int v = a.pdfs[f * a.K + k];
    if (v >= a.D) bad++;
    else if (v >= 0) { d = v; q = a.probs[f * a.K + k]; }
  }
}

// the entries of frame f over its row of e (already stored by this wave)
template <int XH, int VW>
__device__ __forceinline__ void bo_targets(const BoostArgs& a, size_t f, int lane, int& bad) {
  const int K = a.K;
  const size_t row = f * a.D;
  for (int k0 = 0; k0 < K; k0 += 64) {
    int d, none = 0;
    float q;
    bo_entries(a, f, k0, lane, d, q, bad);
    const int k = k0 + lane;
    bool first = d >= 0;
    float qd = q;
    for (int j0 = 0; j0 < K; j0 += 64) {
      int dj = d;
      float qj = q;
      if (j0 != k0) bo_entries(a, f, j0, lane, dj, qj, none);     // (K > 64 only; counted where k0 reaches them)
      const int n = K - j0 < 64 ? K - j0 : 64;
      for (int j = 0; j < n; j++) {
        const int du = lane_int(dj, j);
        const float qu = lane_float(qj, j);
        if (du == d && d >= 0) {
          if (j0 + j < k) first = false;
          else if (j0 + j > k) qd = bo_add(qd, qu);               // ascending k
        }
      }
    }
    const float fac = bo_factor(a.boost, qd);
    const int dd = first ? d : -1;
    const int n = K - k0 < 64 ? K - k0 : 64;
    for (int j = 0; j < n; j++) {
      const int du = lane_int(dd, j);
      if (du < 0) continue;                                       // (wave-uniform)
      const float fu = lane_float(fac, j);
      if (((du / VW) & 63) == lane) {                             // the lane whose dense store wrote this element
        float v[1];
        row_load<XH, 1>(a.x, row + du, v);
        a.e[row + du] = bo_mul(clamp_exp(v[0], kXExpClamp), fu);
      }
    }
  }
}

// XH: x's element type; VW: elements per access, 4 or 1 (1: rows that are no multiple of 4 elements) - row_load<XH, VW> of x,
// row_store<kXF32, VW> of e, row_load<XH, 1> where an entry is applied
template <int XH, int VW>
__global__ __launch_bounds__(kBoNT) void boost_rows_kernel(const BoostArgs a, int nchunk, int nitems) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int T = a.T, D = a.D;
  int bad = 0;
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int b = item / nchunk, t0 = (item - b * nchunk) * kBoChunk + wave * kBoRows;
    const int L = seq_len(a.lengths, b, T);
    if (t0 >= L) continue;                                        // rows beyond the length: neither read nor written
    // the wave's second row; where the sequence ends on the first, that one is read again and nothing is stored for it
    const bool two = t0 + 1 < L;
    const size_t f0 = (size_t)b * T + t0;
    const size_t row0 = f0 * D, row1 = two ? row0 + D : row0;
    bool nan0 = false, nan1 = false;
#pragma unroll 2
    for (int e = lane * VW; e < D; e += 64 * VW) {
      float xa[VW], xb[VW];
      row_load<XH, VW>(a.x, row0 + e, xa);
      row_load<XH, VW>(a.x, row1 + e, xb);
#pragma unroll
      for (int i = 0; i < VW; i++) {
        nan0 = nan0 || xa[i] != xa[i];
        nan1 = nan1 || xb[i] != xb[i];
        xa[i] = clamp_exp(xa[i], kXExpClamp);
        xb[i] = clamp_exp(xb[i], kXExpClamp);
      }
      row_store<kXF32, VW>(a.e, row0 + e, xa);
      if (two) row_store<kXF32, VW>(a.e, row1 + e, xb);
    }
    bo_targets<XH, VW>(a, f0, lane, bad);
    if (two) bo_targets<XH, VW>(a, f0 + 1, lane, bad);
    const bool any0 = __ballot(nan0) != 0, any1 = two && __ballot(nan1) != 0;       // (the whole wave is here: t0, L are uniform)
    if (lane == 0) bad += (any0 ? 1 : 0) + (any1 ? 1 : 0);
  }
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if (lane == 0 && bad != 0) atomicAdd(a.bad_count, bad);         // (an integer sum: the same value in any order)
}

template <int XH>
hipError_t launch_as(const BoostArgs& a, int grid, int nchunk, int nitems, hipStream_t st) {
  if (a.D % 4 == 0) hipLaunchKernelGGL((boost_rows_kernel<XH, 4>), dim3(grid), dim3(kBoNT), 0, st, a, nchunk, nitems);
  else hipLaunchKernelGGL((boost_rows_kernel<XH, 1>), dim3(grid), dim3(kBoNT), 0, st, a, nchunk, nitems);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_boost_rows(const BoostArgs& a, hipStream_t st) {
  const int nchunk = (a.T + kBoChunk - 1) / kBoChunk;
  const size_t items = (size_t)a.B * nchunk;
  if (items > (size_t)INT_MAX || (size_t)a.B * a.T > (size_t)INT_MAX) return hipErrorInvalidValue;
  const int nitems = (int)items, grid = nitems < kRowPassMaxGrid ? nitems : kRowPassMaxGrid;
  hipError_t e = hipMemsetAsync(a.bad_count, 0, sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  if (a.x_half == kXF32) return launch_as<kXF32>(a, grid, nchunk, nitems, st);
  if (a.x_half == kXBf16) return launch_as<kXBf16>(a, grid, nchunk, nitems, st);
  return launch_as<kXF16>(a, grid, nchunk, nitems, st);
}

}  // namespace pychain_hip

using namespace pychain_hip;

// ---- the entry point (include/pychain_hip.h) ------------------------------------------------------------------------------------
extern "C" int pychain_hip_boost_rows(const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
                                      const int32_t* target_pdfs, const float* target_probs, int K, float boost,
                                      float* e, int32_t* bad_count, void* stream) {
  const char* who = "boost_rows";
  if (nnet_output_dtype < PYCHAIN_HIP_F32 || nnet_output_dtype > PYCHAIN_HIP_F16)
    return fail(PYCHAIN_HIP_EINVAL, "%s: unknown nnet_output_dtype %d", who, nnet_output_dtype);
  if (!nnet_output || !seq_lengths || !target_pdfs || !target_probs || !e || !bad_count)
    return fail(PYCHAIN_HIP_EINVAL, "%s: null pointer argument", who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  if (!(boost >= 0.f) || boost > 3.0e38f) return fail(PYCHAIN_HIP_EINVAL, "%s: boost must be finite and not negative, got %g", who, (double)boost);
  if (((uintptr_t)nnet_output | (uintptr_t)e) & 15) return fail(PYCHAIN_HIP_EINVAL, "%s: nnet_output and e must be 16-byte aligned", who);
  BoostArgs a;
  memset(&a, 0, sizeof(a));
  a.x = nnet_output; a.x_half = nnet_output_dtype; a.lengths = seq_lengths; a.pdfs = target_pdfs; a.probs = target_probs;
  a.boost = boost; a.e = e; a.bad_count = bad_count; a.B = B; a.T = T; a.D = D; a.K = K;
  const hipError_t err = launch_boost_rows(a, (hipStream_t)stream);
  if (err != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "%s: %s", who, hipGetErrorString(err));
  return PYCHAIN_HIP_OK;
}
