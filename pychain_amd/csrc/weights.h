// weights.h - launch interface of the utterance / derivative weights pass (weights.hip): the rows of a [B,T,D] gradient scaled
// in place by w(b,t) = u_b * f_bt, and the weighted sums of the per-sequence objectives (include/pychain_hip.h:
// pychain_hip_weight_rows).
#ifndef PYCHAIN_HIP_WEIGHTS_H_
#define PYCHAIN_HIP_WEIGHTS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pychain_hip {

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

// the streaming pass over the live rows whose weight is neither 1 (not touched) nor 0 (zeros stored, nothing loaded)
hipError_t launch_weight_rows(const WeightRowsArgs& a, hipStream_t st);
// one thread, fp64, ascending b, in stream order behind whatever wrote `totals` and the per-sequence arrays
hipError_t launch_weight_sums(const WeightSumsArgs& s, hipStream_t st);

}  // namespace pychain_hip
#endif
