// smbr_general.hip - lattice-free sMBR for graphs and trees the LDS kernels of smbr.hip do not take (DESIGN.md §3.28;
// include/pychain_hip.h: pychain_hip_smbr_forward_backward_general): four state vectors and four rows of a frame beyond the 160 KiB
// of a CU - 3000 states with more than about 7 200 pdfs, identity classes sooner, more than about 10 000 states at any D.  As
// den_general.hip is to the compiled-plan kernels: SLOW - what does not fit LDS is gathered from global memory, L2-resident at
// best - but complete, any H, K, D, C that the int32 reference layout holds, with the decomposition, the workspace layout and the
// checks of smbr.hip, so everything around the two launches is shared.
//
//   smbr_general_recursion_kernel<XH, CLS, VLDS>   2B persistent workgroups of 1024, one per (sequence, direction); a thread owns
//                                  states tid, tid + 1024, ..., arcs in the reference layout: the `recursion` of smbr_device.h.
//                                  The frame's row x = exp(clamp(y)), its companion x A and the class table lie in scratch rows of
//                                  the workspace, the two rows double-buffered and made a frame ahead, as the LDS kernel makes them.
//                                  VLDS ("rows"): both state vectors double-buffered in LDS, 4 H floats.  !VLDS ("global"): the
//                                  previous state rows are read back from the trajectory store the workgroup has just written.
//   smbr_general_grad_kernel<XH, CLS>   at most kSmbrGradMaxWgs workgroups of 512, persistent over the (sequence, block of 8 frames)
//                                  items, each frame by smbr_grad_frame of smbr_device.h; a thread owns pdfs tid, tid + 512, ...;
//                                  the four state rows are gathered straight from the trajectories (written by the launch
//                                  before: plain loads), the two D-rows x q0 and x (q1 + a q0) and the class table lie in
//                                  scratch rows of the workgroup.
//
// Staged rows, not a gather of y per arc: C4's graph has 30 000 arcs on 8408 pdfs, so a gather exp's every element 3.6 times a
// frame and direction on the arc loop's dependent chain, and it would need the frame's K target entries searched per arc (or the
// class table read through a second dependent gather).  The forward workgroup has to pass over all D elements of a live row in any
// case - a NaN on a pdf no arc carries is a NaN loss -, and that pass stages the row for one store more an element.
//
// A value another thread of the workgroup wrote to global memory before the last barrier is read as den_general.hip reads it:
// load_fresh (around the vector L1, which other waves' stores do not refresh) behind `__threadfence(); __syncthreads();` - the
// read and the publish of the storage policies FrameRows and FrameGlobal (smbr_device.h).
//
// SAME BITS.  Thread-to-state and thread-to-pdf ownership, the arc order and the order of every sum are those of smbr.hip - the
// recursion, the gradient frame and the closing are one copy, smbr_device.h, instantiated here over scratch rows -, and this unit
// too is compiled with contraction off: where both run, the general kernels give the bits of the LDS kernels
// (tests/test_gpu_smbr_general.py).  Nothing is atomic but integer counters and flags.
#include <hip/hip_runtime.h>

#include <cstring>

#pragma clang fp contract(off)      // ahead of the project's headers: their inline helpers (clamp_exp, the row loads) are under it too

#include "../../include/pychain_hip.h"
#include "common.h"
#include "row_access.h"
#include "smbr.h"
#include "smbr_device.h"

namespace pychain_hip {
namespace {

// `recursion` (smbr_device.h) with the weighted pair over FrameRows or FrameGlobal: x [2][D], x A [2][D] and Acls [C] in the
// workgroup's scratch row; lds: red [kSmRed], then with VLDS the state vectors [2][H], [2][H]
template <int XH, bool CLS, bool VLDS>
__global__ __launch_bounds__(kSmNT) void smbr_general_recursion_kernel(const SmbrArgs a, const SmbrClasses c, const SmbrGeneral s) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  using S = std::conditional_t<VLDS, FrameRows, FrameGlobal>;
  const size_t H = a.g.H, D = a.D;
  RecArgs r = smbr_rec_args(a);
  r.red = lds; r.vec0 = lds + kSmRed; r.vec1 = r.vec0 + 2 * H;
  r.xrow = s.rec + (size_t)blockIdx.x * s.rec_stride; r.xacc = r.xrow + 2 * D; r.acl = r.xacc + 2 * D;
  if (blockIdx.x < (unsigned)a.B) recursion<XH, true, CLS, true, S>(r, c, blockIdx.x);
  else recursion<XH, false, CLS, true, S>(r, c, blockIdx.x - a.B);
}

// smbr_grad_frame (smbr_device.h) over FrameGlobal: the state rows read where the recursions left them, x q0 [D], x (q1 + a q0) [D]
// and Acls [C] in the workgroup's scratch row; persistent over the (sequence, block of frames) items, the first of a sequence
// closes it
template <int XH, bool CLS>
__global__ __launch_bounds__(kSmGNT) void smbr_general_grad_kernel(const SmbrArgs a, const SmbrClasses c, const SmbrGeneral s) {
  __shared__ float red[kSmRed];
  float* const gq = s.grad + (size_t)blockIdx.x * s.grad_stride;
  float* const gv = gq + a.D;
  const float gscale = a.grad_scale_dev ? a.grad_scale * *a.grad_scale_dev : a.grad_scale;
  const int nblk = (a.T + kSmFrames - 1) / kSmFrames;
  const int items = a.B * nblk;
  for (int it = blockIdx.x; it < items; it += gridDim.x) {
    const int b = it / nblk, blk = it - b * nblk;
    const int L = seq_len(a.lengths, b, a.T);
    const int t_begin = blk * kSmFrames, t_end = min(t_begin + kSmFrames, a.T);
    for (int t = t_begin; t < t_end; t++) smbr_grad_frame<XH, CLS, FrameGlobal>(a, c, b, t, L, gscale, nullptr, gq, gv, gv + a.D, red);
    if (blk == 0) {
      smbr_close(a, b, L, red);
      __syncthreads();                                                         // (red is free for the next item)
    }
  }
}

// the recursion launch of the form, then the gradient launch
template <int XH, bool CLS>
hipError_t launch_as(const SmbrArgs& a, const SmbrClasses& c, const SmbrGeneral& s, hipStream_t st) {
  const size_t lds = (kSmRed + (s.state_lds ? 4 * (size_t)a.g.H : 0)) * sizeof(float);
  const hipError_t e = s.state_lds ? launch_with_lds(smbr_general_recursion_kernel<XH, CLS, true>, dim3(2 * a.B), dim3(kSmNT), lds, st, a, c, s)
                                   : launch_with_lds(smbr_general_recursion_kernel<XH, CLS, false>, dim3(2 * a.B), dim3(kSmNT), lds, st, a, c, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((smbr_general_grad_kernel<XH, CLS>), dim3(s.grad_wgs), dim3(kSmGNT), 0, st, a, c, s);
  return hipGetLastError();
}

size_t round64(size_t floats) { return (floats + 63) & ~size_t(63); }

}  // namespace

size_t smbr_general_lds(int H) { return (4 * (size_t)H + kSmRed) * sizeof(float) + kSmStaticLds; }
size_t smbr_general_rec_stride(int D, int C) { return round64(4 * (size_t)D + (size_t)C); }
size_t smbr_general_grad_stride(int D, int C) { return round64(2 * (size_t)D + (size_t)C); }
int smbr_general_grad_wgs(int B, int T) {
  const size_t items = (size_t)B * ((T + kSmFrames - 1) / kSmFrames);
  return (int)(items < (size_t)kSmbrGradMaxWgs ? items : (size_t)kSmbrGradMaxWgs);
}

hipError_t launch_smbr_general(const SmbrArgs& a, const SmbrClasses& c, const SmbrGeneral& s, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.seq_bad, 0, 2 * (size_t)a.B * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  return by_row_dtype(a.x_half, [&](auto xh) {
    constexpr int XH = decltype(xh)::value;
    return c.cls ? launch_as<XH, true>(a, c, s, st) : launch_as<XH, false>(a, c, s, st);
  });
}

}  // namespace pychain_hip
