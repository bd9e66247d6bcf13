// row_access.h - the element access of the memory-bound passes over [B,T,D] rows (outreg.hip, weights.hip, post.hip, boost.hip,
// the row kernel of xent.hip): VW elements at an element offset, fp32 / bf16 / fp16, widened to fp32 (exact), and the matching
// store that rounds to nearest even (device_utils.h: f32_to_half_bits).  The headers of those files count these roundings; this
// is their one copy.  Beside it what the passes share on the host: the cap of their strided grids and the dtype x width ladder.
#ifndef PYCHAIN_HIP_ROW_ACCESS_H_
#define PYCHAIN_HIP_ROW_ACCESS_H_

#include <type_traits>
#include <utility>

#include "device_utils.h"

namespace pychain_hip {

constexpr int kRowPassMaxGrid = 2048;               // 256 CUs x 8 workgroups: the rest is strided over

// VW elements at element offset e: 16 bytes (fp32 x 4, 2-byte x 8), 8 bytes (2-byte x 4) or one element
template <int XH, int VW>
__device__ __forceinline__ void row_load(const void* p, size_t e, float (&v)[VW]) {
  if constexpr (XH == kXF32) {
    static_assert(VW == 4 || VW == 1, "fp32 rows: float4 or one element");
    if constexpr (VW == 4) {
      const float4 q = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + e);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = reinterpret_cast<const float*>(p)[e];
    }
  } else {
    static_assert(VW == 8 || VW == 4 || VW == 1, "2-byte rows: eight, four or one element");
    constexpr bool BF = XH == kXBf16;
    const uint16_t* h = reinterpret_cast<const uint16_t*>(p) + e;
    if constexpr (VW == 8) {
      const uint4 q = *reinterpret_cast<const uint4*>(h);
      half2_to_f32(q.x, BF, v[0], v[1]); half2_to_f32(q.y, BF, v[2], v[3]);
      half2_to_f32(q.z, BF, v[4], v[5]); half2_to_f32(q.w, BF, v[6], v[7]);
    } else if constexpr (VW == 4) {
      const uint2 q = *reinterpret_cast<const uint2*>(h);
      half2_to_f32(q.x, BF, v[0], v[1]); half2_to_f32(q.y, BF, v[2], v[3]);
    } else {
      v[0] = half_bits_to_f32(*h, BF);
    }
  }
}
template <int XH, int VW>
__device__ __forceinline__ void row_store(void* p, size_t e, const float (&v)[VW]) {
  if constexpr (XH == kXF32) {
    if constexpr (VW == 4) *reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + e) = make_float4(v[0], v[1], v[2], v[3]);
    else reinterpret_cast<float*>(p)[e] = v[0];
  } else {
    constexpr bool BF = XH == kXBf16;
    uint16_t* h = reinterpret_cast<uint16_t*>(p) + e;
    if constexpr (VW == 8) {
      uint4 q;
      q.x = pack_half2(v[0], v[1], BF); q.y = pack_half2(v[2], v[3], BF);
      q.z = pack_half2(v[4], v[5], BF); q.w = pack_half2(v[6], v[7], BF);
      *reinterpret_cast<uint4*>(h) = q;
    } else if constexpr (VW == 4) {
      uint2 q;
      q.x = pack_half2(v[0], v[1], BF); q.y = pack_half2(v[2], v[3], BF);
      *reinterpret_cast<uint2*>(h) = q;
    } else {
      *h = (uint16_t)f32_to_half_bits(v[0], BF);
    }
  }
}
// Four elements, the address formed at the store and not ahead of the packing.  The same operations as row_store<XH, 4>; the
// compiler schedules the two differently, and the row kernel of xent.hip keeps the code it had only in this shape.
template <int XH>
__device__ __forceinline__ void row_store4_late(void* p, size_t e, const float (&v)[4]) {
  if constexpr (XH == kXF32) {
    row_store<XH, 4>(p, e, v);
  } else {
    uint2 q;
    q.x = pack_half2(v[0], v[1], XH == kXBf16); q.y = pack_half2(v[2], v[3], XH == kXBf16);
    *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p) + e) = q;
  }
}
// One element, by value: what row_load<XH, 1> / row_store<XH, 1> do, written out.  (As wrappers of those, or with those calling
// these, one fp16 kernel of xent.hip or of outreg.hip comes out with its instructions in another order.)
template <int XH>
__device__ __forceinline__ float row_load1(const void* p, size_t e) {
  if constexpr (XH == kXF32) return reinterpret_cast<const float*>(p)[e];
  else return half_bits_to_f32(reinterpret_cast<const uint16_t*>(p)[e], XH == kXBf16);
}
template <int XH>
__device__ __forceinline__ void row_store1(void* p, size_t e, float v) {
  if constexpr (XH == kXF32) reinterpret_cast<float*>(p)[e] = v;
  else reinterpret_cast<uint16_t*>(p)[e] = (uint16_t)f32_to_half_bits(v, XH == kXBf16);
}

// fp64 sum over the wave by the xor butterfly 32, 16, .. 1: every lane ends with the same bits
__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The dtype x width ladder of a pass whose rows start 16-byte aligned: f(integral_constant<int, XH>, integral_constant<int, VW>)
// with the widest VW that divides D - fp32: 4, else 1; 2-byte: 8, 4, else 1.  xh is kXF32, kXBf16 or kXF16 (the caller checked).
template <int XH, class F>
auto row_width_dispatch_as(int D, F&& f) {
  using X = std::integral_constant<int, XH>;
  if constexpr (XH != kXF32) {
    if (D % 8 == 0) return f(X(), std::integral_constant<int, 8>());
  }
  if (D % 4 == 0) return f(X(), std::integral_constant<int, 4>());
  return f(X(), std::integral_constant<int, 1>());
}
template <class F>
auto row_width_dispatch(int xh, int D, F&& f) {
  if (xh == kXF32) return row_width_dispatch_as<kXF32>(D, std::forward<F>(f));
  if (xh == kXBf16) return row_width_dispatch_as<kXBf16>(D, std::forward<F>(f));
  return row_width_dispatch_as<kXF16>(D, std::forward<F>(f));
}

}  // namespace pychain_hip
#endif
