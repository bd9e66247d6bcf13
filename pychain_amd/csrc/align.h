// align.h - launch interface of the Viterbi alignment kernels (align.hip).
#ifndef PYCHAIN_HIP_ALIGN_H_
#define PYCHAIN_HIP_ALIGN_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pychain_hip {

struct AlignArgs {
  const int32_t* bwd_trans; const int32_t* bwd_idx; const float* bwd_probs;   // arcs entering each state, [G,K,3] / [G,H,2] / [G,K]
  const float* initial; const float* final_;                                  // [G,H] log
  const float* x;            // [B,T,D] raw   (x_half: 2-byte elements behind this pointer)
  int x_half;                // 0 fp32; kXBf16 / kXF16 (device_utils.h): tile kernels only
  const int64_t* lengths;    // [B]
  double* score;             // [B]    best-path log-score, final weight included; NaN / -inf = not ok
  int32_t* states;           // [B,T+1]
  int64_t* pdfs;             // [B,T]
  int32_t* bad;              // [1]    utterances not ok (+ lengths outside [1, T])
  uint16_t* bp16;            // tile:    [B,T,Hb] offset of the winning arc inside [lo, hi) of its destination
  int32_t* bp32;             // general: [B,T,H]
  double* gen_sc;            // general: [B,2,H] ping-pong score vectors
  int graph_stride;          // 1 = per-sequence graphs, 0 = shared
  int B, T, D, H, K;
  int Hb;                    // row stride of bp16 (H rounded up to even: rows are read back as 32-bit words)
  int walk_bytes;            // tile: LDS bytes of the region the backtrace stages rows in (>= the score + row buffers it reuses)
  int general;               // graphs beyond the tile kernels (num_needs_general)
  const int32_t* windows;    // [B,H,2] {lo, hi} alignment time windows (pychain_hip_align_tw), nullptr = none
};

int align_walk_bytes(int H, int K, int D);
size_t align_lds_bytes(int H, int K, int D);
hipError_t launch_align(const AlignArgs& a, hipStream_t st, const char** why);

}  // namespace pychain_hip
#endif
