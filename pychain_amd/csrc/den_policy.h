// den_policy.h - what a denominator call runs and in which order (den_policy.hip): the recursion family of a call, the DenArgs a
// query entry point asks with, the schedules of the recursion and occupancy launches, the library's side streams.
#ifndef PYCHAIN_HIP_DEN_POLICY_H_
#define PYCHAIN_HIP_DEN_POLICY_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "den_kernels.h"

namespace pychain_hip {

inline int roundup64(int x) { return (x + 63) / 64 * 64; }
int device_cu_count();               // of the current device (cached); 256 where there is none

// ---- library-owned side streams (the only hidden state besides the option table): one for the numerator
// recursion, one for the occupancy launches that overlap the denominator recursion ------------------
constexpr int kMaxSegments = 16;
struct SideStream {
  hipStream_t stream = nullptr, stream2 = nullptr;
  hipEvent_t fork = nullptr, join = nullptr, seg[kMaxSegments] = {}, join2 = nullptr;
  bool ready = false;       // every stream and event below was created
};
SideStream* side_streams_for(hipStream_t caller);      // null: they could not be created

// The sizes, the calling thread's settings and what follows from them alone, into a zeroed `a`: what a call (api.hip:
// fill_den_args) and a query share.
void den_shape_args(DenArgs& a, int64_t plan_stride, int H, int D, int B, int T);
// THE decision of a call's recursion family: sets a.pair, a.lazy, a.shape, a.sg from the sizes, plan stride, fused, input_is_exp,
// x_half, knobs and the hint - nothing else writes them.  The stored rows of a forward call are only readable by a later
// chain_loss_backward if both decide alike (DenArgs::lazy, DenArgs::sg), and what callers allocate follows the queries.
void den_decide_family(DenArgs& a, int hint);
// The DenArgs of a query entry point, decided: a query cannot answer from a half-filled struct.
DenArgs den_query_args(int64_t plan_stride, int hint, int H, int D, int B, int T, bool fused, bool input_is_exp = false);

int den_time_segments(const DenArgs& a, bool fused);   // (a decided)
bool den_would_exp_rows_ahead(const DenArgs& a);       // (a decided)
bool den_call_half_native(const DenArgs& a, int hint); // (a as filled: decides on a copy)

// recursion + occupancy launches of one denominator call; run_den: ... and den_finish_kernel behind them
hipError_t run_den_launches(DenArgs& a, int hint, bool occupancy, hipStream_t st, const char** why,
                            hipEvent_t gamma_wait, hipEvent_t zeroed = nullptr, bool* finish_early = nullptr);
hipError_t run_den(DenArgs& a, int hint, bool occupancy, hipStream_t st, const char** why, hipEvent_t gamma_wait = nullptr);

}  // namespace pychain_hip
#endif
