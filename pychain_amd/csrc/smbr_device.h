// smbr_device.h - device code the two sMBR translation units share (smbr.hip: the kernels that keep a frame in LDS; smbr_general.hip:
// the general kernels): the workgroup shapes, the block sum, the ownership of a frame's target entries, the class
// table, the staging of a network-output row and the verdict of a sequence.  The general kernels give the bits of the LDS kernels
// BECAUSE these are one copy: the same partial sums in the same order, the same owner of every entry.  Include it behind
// `#pragma clang fp contract(off)`, as both units do.
#ifndef PYCHAIN_HIP_SMBR_DEVICE_H_
#define PYCHAIN_HIP_SMBR_DEVICE_H_

#include <hip/hip_runtime.h>

#include "device_utils.h"
#include "row_access.h"
#include "smbr.h"

namespace pychain_hip {
namespace {

constexpr int kSmNT = 1024;                 // recursion workgroup: 16 waves
constexpr int kSmGNT = 512;                 // gradient workgroup
constexpr int kSmFrames = 8;                // frames of one gradient workgroup
constexpr int kSmXR = 4;                    // elements of the next row a recursion thread holds in registers across the arc loop
constexpr int kSmRed = 64;                  // floats of reduction scratch
static_assert(48 + kSmGNT / 64 <= kSmRed, "smbr_grad_kernel sums the row mean over red[48 ..], behind block_sum3's 3 x 16");
constexpr size_t kSmStaticLds = 256;        // what the recursion kernel holds beside its dynamic LDS (the closing vote)

// up to three sums over the workgroup, every thread gets the totals; `red` (3 x 16 floats) is free again behind the NEXT barrier
template <int NT>
__device__ __forceinline__ void block_sum3(float& s0, float& s1, float& s2, float* red, int tid) {
  s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
  if ((tid & 63) == 0) { red[tid >> 6] = s0; red[16 + (tid >> 6)] = s1; red[32 + (tid >> 6)] = s2; }
  __syncthreads();
  s0 = s1 = s2 = 0.f;
  for (int w = 0; w < NT / 64; w++) { s0 += red[w]; s1 += red[16 + w]; s2 += red[32 + w]; }     // (same order in every thread)
}

// Entry k of a frame (pd, pr: its Kt entries): true where this thread owns it, with (pdf, summed q).  An entry is handled where
// its pdf occurs first in the frame, q summed in ascending k, so a repeated pdf has one owner and nothing is atomic.
__device__ __forceinline__ bool owned_entry(const int32_t* pd, const float* pr, int k, int Kt, int D, int& d, float& q) {
  d = pd[k];
  if (d < 0 || d >= D) return false;
  for (int j = 0; j < k; j++)
    if (pd[j] == d) return false;
  q = pr[k];
  for (int j = k + 1; j < Kt; j++)
    if (pd[j] == d) q += pr[j];
  return true;
}
// x A of a frame over its zeroed companion row
__device__ __forceinline__ void scatter_entries(const int32_t* pd, const float* pr, int Kt, int D, int tid, int nt, const float* xrow, float* xacc) {
  int d;
  float q;
  for (int k = tid; k < Kt; k += nt)
    if (owned_entry(pd, pr, k, Kt, D, d, q)) xacc[d] = xrow[d] * q;
}

// ---- accuracy by class (§3.27) ----------------------------------------------------------------------------------------------------
// the class of a target id, -1 where it adds nothing: padding, a pdf >= D, a class >= C
__device__ __forceinline__ int entry_class(const SmbrClasses& c, int id, int D) {
  if (id < 0) return -1;
  if (c.targets_are_classes) return id < c.C ? id : -1;
  return id < D ? c.cls[id] : -1;
}
// Acls(t, .) of a frame into `acl` [C]: thread tid, tid + nt, ... sums the q of its class in ascending k - one owner, no atomics
__device__ __forceinline__ void class_table(const SmbrClasses& c, const int32_t* pd, const float* pr, int Kt, int D, int tid, int nt, float* acl) {
  for (int cc = tid; cc < c.C; cc += nt) {
    float q = 0.f;
    for (int k = 0; k < Kt; k++)
      if (entry_class(c, pd[k], D) == cc) q += pr[k];
    acl[cc] = q;
  }
}

// ---- the frame's row ------------------------------------------------------------------------------------------------------------
// row t of the sequence into `lds` (LDS, or a scratch row of the general kernels) as exp(clamp(.)); elements tid + i * NT,
// i < kSmXR, come from `held` (loaded before the arc loop)
template <int XH>
__device__ __forceinline__ void hold_row(const void* x, size_t row, int D, int tid, float (&held)[kSmXR]) {
#pragma unroll
  for (int i = 0; i < kSmXR; i++) {
    const int n = tid + i * kSmNT;
    held[i] = n < D ? row_load1<XH>(x, row + n) : 0.f;
  }
}
template <int XH>
__device__ __forceinline__ bool put_row(const void* x, size_t row, int D, int tid, const float (&held)[kSmXR], float* lds) {
  bool nan = false;
#pragma unroll
  for (int i = 0; i < kSmXR; i++) {
    const int n = tid + i * kSmNT;
    if (n < D) { nan = nan || held[i] != held[i]; lds[n] = clamp_exp(held[i], kXExpClamp); }
  }
  for (int n = tid + kSmXR * kSmNT; n < D; n += kSmNT) {       // (rows of more than 4096 pdfs)
    const float r = row_load1<XH>(x, row + n);
    nan = nan || r != r;
    lds[n] = clamp_exp(r, kXExpClamp);
  }
  return nan;
}

// ---- the verdict ----------------------------------------------------------------------------------------------------------------
// The sequence went bad: its E_b becomes NaN and it is counted ONCE, by whichever workgroup of the gradient launch finds it first
// (seq_bad[B + b]: claimed by an integer compare-and-swap; the same values whoever wins).
__device__ __forceinline__ void smbr_condemn(const SmbrArgs& a, int b) {
  if (atomicCAS(a.seq_bad + a.B + b, 0, 1) == 0) {
    a.acc_per_seq[b] = __builtin_nan("");
    atomicAdd(a.bad_count, 1);                                                 // (an integer count)
  }
}

}  // namespace
}  // namespace pychain_hip
#endif
