// post.h - launch interface of posterior-target supervision (post.hip): sparse per-frame posterior targets as the numerator
// behind a denominator call, and the top-k rows that make such targets out of dense posteriors (include/pychain_hip.h:
// pychain_hip_post_targets, pychain_hip_topk_rows).
#ifndef PYCHAIN_HIP_POST_H_
#define PYCHAIN_HIP_POST_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pychain_hip {

struct PostArgs {
  const void* x;             // [B,T,D] raw, x_half: 0 fp32, kXBf16 / kXF16 (device_utils.h)
  int x_half;
  void* grad;                // [B,T,D] in x's type, or nullptr: the objective only
  const int32_t* pdfs;       // [B,T,K]: < 0 padding, >= D counted as bad
  const float* probs;        // [B,T,K]
  const int64_t* lengths;    // [B]
  float scale;               // s = scale [* *scale_dev] [/ *norm_dev]
  const float* scale_dev;
  const float* norm_dev;
  double* frame_sums;        // [B,T] scratch: sum_k q_k clamp(x) of every live frame
  int32_t* frame_bad;        // [B,T] scratch: entries with pdf >= D of every live frame
  double* seq_sums;          // [B] scratch: the unrounded per-sequence sums
  int32_t* seq_bad;          // [B] scratch
  float* num_objf;           // [B] out
  int B, T, D, K;
};

size_t post_workspace_bytes(int B, int T);
// one thread per frame (objective, gradient), then the per-sequence sums of the frame values in fp64, fixed order
hipError_t launch_post_frames(const PostArgs& a, hipStream_t st);
// one thread: *bad_count = the bad entries; totals (or nullptr): [3] = S = sum den - sum num, [0] = [4] = loss_scale S [/ *norm_dev],
// [2] += the bad entries
hipError_t launch_post_totals(const double* seq_sums, const int32_t* seq_bad, int B, const float* den_objf, float loss_scale,
                              const float* norm_dev, int32_t* bad_count, float* totals, hipStream_t st);

struct TopkArgs {
  const void* rows;          // [B,T,D], dtype as x_half above
  int dtype;
  const int64_t* lengths;
  int32_t* out_pdfs;         // [B,T,K]
  float* out_probs;          // [B,T,K]
  float floor;
  int normalize;
  int B, T, D, K;
};
constexpr int kTopkMaxK = 64;
constexpr int kTopkChipRow = 9216;          // the longest row held in LDS (the fast path's limit); longer rows are re-read
hipError_t launch_topk_rows(const TopkArgs& a, hipStream_t st);

}  // namespace pychain_hip
#endif
