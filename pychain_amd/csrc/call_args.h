// call_args.h - host only: what the entry points of the C ABI (api.hip, align.hip, the host twins of cpu.cpp) pack their
// argument lists into once, the pointer arithmetic from one sequence of a batch to another, and the refusals they share.
#ifndef PYCHAIN_HIP_CALL_ARGS_H_
#define PYCHAIN_HIP_CALL_ARGS_H_

#include <cstddef>
#include <cstdint>

#include "../../include/pychain_hip.h"
#include "common.h"

namespace pychain_hip {

// The numerator graphs of a call: [G,K,3] / [G,H,2] / [G,K] arcs leaving (f*) and entering (b*) each state, [G,H] initial and
// final log-probabilities; stride 1 = a graph per sequence (G = B), 0 = one graph for all.
struct NumGraphs {
  const int32_t* ft; const int32_t* fi; const float* fp;
  const int32_t* bt; const int32_t* bi; const float* bp;
  const float* initial; const float* final_;
  int stride, H, K;
  bool any_null() const { return !ft || !fi || !fp || !bt || !bi || !bp || !initial || !final_; }
  // the graphs from sequence b on
  NumGraphs at(int b) const {
    const size_t g = stride ? (size_t)b : 0;
    NumGraphs s = *this;
    s.ft += g * K * 3; s.fi += g * H * 2; s.fp += g * K;
    s.bt += g * K * 3; s.bi += g * H * 2; s.bp += g * K;
    s.initial += g * H; s.final_ += g * H;
    return s;
  }
};

// The network output of a call, [B,T,D] in `dtype` (PYCHAIN_HIP_F32 / _BF16 / _F16), and the lengths of its sequences.
struct Rows {
  const void* x; int dtype; const int64_t* lengths; int B, T, D;
  size_t elem_bytes() const { return dtype == PYCHAIN_HIP_F32 ? 4 : 2; }
  // bytes from sequence 0 to sequence b0 - of `x` and of every tensor of its shape and dtype (the gradient)
  size_t offset(int b0) const { return (size_t)b0 * T * D * elem_bytes(); }
  Rows slice(int b0, int nb) const {
    Rows s = *this;
    s.x = (const char*)x + offset(b0); s.lengths = lengths + b0; s.B = nb;
    return s;
  }
};

// A caller-owned device workspace; every carve starts from its 256-aligned base.
struct Workspace { void* p; size_t bytes; };
inline char* ws_base(void* workspace) { return (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255); }

// the time windows of sequence b ([B,H,2]: one row per sequence, shared graph or not); nullptr = none
inline const int32_t* window_row(const int32_t* windows, int b, int H) { return windows ? windows + (size_t)b * H * 2 : nullptr; }

// ---- the refusals the entry points share (`who`: the entry point as its messages name it) ----
inline int null_pointer(const char* who) { return fail(PYCHAIN_HIP_EINVAL, "%s: null pointer argument", who); }
inline int bad_dtype(const char* who, int dtype) {
  if (dtype >= PYCHAIN_HIP_F32 && dtype <= PYCHAIN_HIP_F16) return PYCHAIN_HIP_OK;
  return fail(PYCHAIN_HIP_EINVAL, "%s: unknown nnet_output_dtype %d", who, dtype);
}
inline int bad_stride(const char* who, int stride) {
  if (stride == 0 || stride == 1) return PYCHAIN_HIP_OK;
  return fail(PYCHAIN_HIP_EINVAL, "%s: graph_batch_stride must be 0 or 1", who);
}
inline int bad_sizes(const char* who, int B, int T, int H, int K, int D) {
  if (B > 0 && T > 0 && H > 0 && K > 0 && D > 0) return PYCHAIN_HIP_OK;
  return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d H=%d K=%d D=%d", who, B, T, H, K, D);
}
inline int bad_sizes(const char* who, const Rows& r, const NumGraphs& g) { return bad_sizes(who, r.B, r.T, g.H, g.K, r.D); }

#ifdef HIP_INCLUDE_HIP_HIP_RUNTIME_H        // (the .hip files, which include the runtime's header first; cpu.cpp launches nothing)
// a launch that did not go through: `why` where a launcher declined the shape, else the runtime's error
inline int launch_failed(const char* who, hipError_t e, const char* why) {
  return fail(why ? PYCHAIN_HIP_EUNSUPPORTED : PYCHAIN_HIP_ELAUNCH, "%s: %s", who, why ? why : hipGetErrorString(e));
}
#endif

}  // namespace pychain_hip
#endif
