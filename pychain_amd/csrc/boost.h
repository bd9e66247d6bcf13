// boost.h - launch interface of the boosted denominator's row pass (boost.hip): e = exp(clamp(x)) with the elements a frame's
// sparse targets address scaled by exp(-boost * a) (include/pychain_hip.h: pychain_hip_boost_rows).
#ifndef PYCHAIN_HIP_BOOST_H_
#define PYCHAIN_HIP_BOOST_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pychain_hip {

struct BoostArgs {
  const void* x;             // [B,T,D] raw, x_half: 0 fp32, kXBf16 / kXF16 (device_utils.h)
  int x_half;
  const int64_t* lengths;    // [B]
  const int32_t* pdfs;       // [B,T,K]: < 0 padding, >= D counted as bad
  const float* probs;        // [B,T,K]
  float boost;
  float* e;                  // [B,T,D] out, fp32; rows t >= L_b are not written
  int32_t* bad_count;        // [1], zeroed on the stream before the launch; the kernel adds to it
  int B, T, D, K;
};

// a wave per row, two rows in flight per wave; the frame's entries applied behind the dense store by the lane that stored the element
hipError_t launch_boost_rows(const BoostArgs& a, hipStream_t st);

}  // namespace pychain_hip
#endif
