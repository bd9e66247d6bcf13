// xent.h - launch interface of the cross-entropy row kernel (xent.hip): the numerator posteriors of a call as targets of a
// second network output (include/pychain_hip.h: pychain_hip_xent).
#ifndef PYCHAIN_HIP_XENT_H_
#define PYCHAIN_HIP_XENT_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pychain_hip {

struct XentArgs {
  const void* z;             // [B,T,D] raw, z_half: 0 fp32, kXBf16 / kXF16 (device_utils.h): 2-byte rows are read as they are
  int z_half;
  void* grad;                // [B,T,D] in z's type, or nullptr: the form without the store
  float scale;               // grad = scale [* *scale_dev] [/ *norm_dev] * (gamma - s softmax(z))
  const float* scale_dev;
  const float* norm_dev;
  const int64_t* lengths;    // [B]
  const double* logp;        // [B] the numerator's log-probabilities (NumArgs::logp_ws): not finite = gamma 0
  // gamma, one of: the compact rows of the tile path (NumArgs::rows_ws / upd_ws / ucount_ws, rows of K words) ...
  const float* rows; const int32_t* upd; const int32_t* ucount; int K;
  const float* dense;        // ... or dense fp32 rows [B,T,D] (numerator graphs on the general kernels)
  // ... or sparse entries [B,T,K] (pychain_hip_xent_targets: posterior targets; K above is then the entries per frame, logp is
  // nullptr - every sequence has targets -, and frame_bad [B,T] receives the entries with pdf >= D of every live frame)
  const int32_t* tpdfs; const float* tprobs; int32_t* frame_bad; int32_t* seq_bad;
  double* frame_objf;        // [B,T] scratch: the objective of every frame
  float* objf;               // [B] out
  int B, T, D;
};

size_t xent_frame_bytes(int B, int T);
// one workgroup per frame (live frames: the row of z once, the gradient row once; frames beyond a length: zeros), then the
// per-sequence sums of the frame objectives in fp64, fixed order
hipError_t launch_xent_rows(const XentArgs& a, hipStream_t st, const char** why);
// xent_totals[0] = loss_scale * S [/ *norm_dev], [1] = S = sum_b objf[b]; totals (or nullptr): [0] = [4] = totals[0] + coef * xent_totals[0],
// [2] += *bad_count (or nullptr)
hipError_t launch_xent_totals(const float* objf, int B, float loss_scale, const float* norm_dev, float coef, float* xent_totals,
                              float* totals, hipStream_t st, const int32_t* bad_count = nullptr);
// the event that joins the row kernel on a side stream back to the caller's stream (one per device and caller stream)
hipEvent_t xent_join_event(hipStream_t caller);

}  // namespace pychain_hip
#endif
