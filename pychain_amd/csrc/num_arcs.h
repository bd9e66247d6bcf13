// num_arcs.h - launch interface of the numerator's arc-weight and arc-count kernels (num_arcs.hip).
#ifndef PYCHAIN_HIP_NUM_ARCS_H_
#define PYCHAIN_HIP_NUM_ARCS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "num_kernels.h"

namespace pychain_hip {

constexpr int kNumArcFrames = 64;          // frames of a count workgroup's run: one partial row [K] of doubles per run

// num_arc_weight_kernel: the caller's graphs (graph_stride 0 or 1) -> lp + w of every sequence in both arc orders and, for a
// shared graph, a copy per sequence of the arrays the probabilities are indexed with (the recursion kernels step from one
// sequence's graph to the next by ONE stride: B probability buffers need B of everything)
struct NumArcWeightArgs {
  const int32_t* ft; const int32_t* fi; const float* fp;
  const int32_t* bt; const int32_t* bi; const float* bp;
  const float* initial; const float* final_;
  int graph_stride, B, H, K;
  const float* w;                          // [B,K] arc log-weights in the forward order
  float* wf; float* wb;                    // [B,K] out: fl32(lp + w) in the forward / in the backward order
  int32_t* rft; int32_t* rfi; int32_t* rbt; int32_t* rbi; float* rinit; float* rfin;    // [B,...] copies, or null (graph_stride 1)
  int32_t* bad;                            // the weights that are not finite
};
hipError_t launch_num_arc_weights(const NumArcWeightArgs& w, hipStream_t st);

// num_arc_count_kernel + num_arc_reduce_kernel over what the recursions of `n` left in the workspace
struct NumArcArgs {
  NumArgs n;
  double* partial;                         // workspace: [B][nrun][K]
  double* counts;                          // [B,K] out
  double* objf;                            // [B] out: logp_ws
  int nrun;                                // ceil(T / kNumArcFrames)
};
// the LDS-staged form keeps one fp32 row of log state occupancies: where it fits, unless `gather` asks for the other form
bool num_arc_count_staged(int H, bool gather);
hipError_t launch_num_arc_counts(const NumArcArgs& c, bool gather, hipStream_t st);

}  // namespace pychain_hip
#endif
