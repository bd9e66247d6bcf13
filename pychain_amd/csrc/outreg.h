// outreg.h - launch interface of the output regularisers (outreg.hip): output L2 and the out-of-range penalty over the
// network output itself (include/pychain_hip.h: pychain_hip_output_reg).
#ifndef PYCHAIN_HIP_OUTREG_H_
#define PYCHAIN_HIP_OUTREG_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pychain_hip {

enum { kRegNoGrad = 0, kRegAccum = 1, kRegLinear = 2 };

struct OutRegArgs {
  const void* x;             // [B,T,D] raw, x_half: 0 fp32, kXBf16 / kXF16 (device_utils.h): 2-byte rows are read as they are
  int x_half;
  void* grad;                // [B,T,D] in x's type, or nullptr (mode kRegNoGrad)
  int mode;
  float l2, oor, limit;
  float scale;               // s = scale [* *scale_dev] [/ *norm_dev]
  const float* scale_dev;
  const float* norm_dev;
  const int64_t* lengths;    // [B]
  double* frame_pairs;       // [B,T,2] scratch: {sum x^2, sum e^2} of every live frame
  double* seq_pairs;         // [B,2] scratch: the unrounded per-sequence sums
  float* per_seq;            // [B,2] out
  int B, T, D;
};

size_t outreg_workspace_bytes(int B, int T);
// the streaming pass over the live rows, then the per-sequence sums of the frame pairs in fp64, fixed order
hipError_t launch_outreg_rows(const OutRegArgs& a, hipStream_t st);
// reg_totals[0] = loss_scale * (0.5 l2 S2 + oor SO) [/ *norm_dev], [1] = S2, [2] = SO; totals (or nullptr): [0] and [4] += that
hipError_t launch_outreg_totals(const double* seq_pairs, int B, float l2, float oor, float loss_scale, const float* norm_dev,
                                float* reg_totals, float* totals, hipStream_t st);

}  // namespace pychain_hip
#endif
