// post.hip - posterior-target supervision (include/pychain_hip.h: pychain_hip_post_targets, pychain_hip_topk_rows; DESIGN.md
// §3.22).  The numerator of the chain objective is not a graph here but a set of sparse per-frame posterior targets q(b,t,k) on
// pdfs pdf(b,t,k) - from a teacher model, or lattice posteriors of unlabelled audio (Kaldi's "KL" objective):
//   num_b = sum_{t<L_b} sum_k q_k clamp(x(b,t,pdf_k), -30, 30),      d num_b / dx(b,t,d) = sum_{k: pdf_k == d} q_k
// behind a denominator call that has left grad = s' gamma_den and its totals on the same stream.
//
// post_frames_kernel: ONE THREAD OWNS A FRAME.  It reads the frame's K entries, gathers the K elements of x they address, and -
// with a gradient - reads, updates and writes exactly the addressed elements of the stored gradient row.  A pdf that occurs
// several times in a frame is handled where it occurs first (the later q are added to the first, ascending k), so nothing
// races and nothing is atomic.  Rows and entries t >= L_b are never read.  The pass moves B T K (8 + sizeof x [+ 2 sizeof x])
// bytes - at K = 8 a four-hundredth of one pass over a row of 3456 pdfs.
//
// THE OPERATION SEQUENCE.  Objective, fp64 from the widening on:
//     c   = clamp((double)x, -30, 30)          exact; a NaN stays a NaN
//     acc = fma((double)q, c, acc)             q c is exact in fp64 (24 x 24 bits): one rounding, the add; k ascending
// one value per live frame into the workspace; post_seq_sum_kernel adds the frames of a sequence (thread by thread in
// ascending t, xor butterfly, the four waves pairwise) and rounds to fp32 ONCE; post_totals_kernel adds the float denominator
// objectives and the unrounded numerator sums in ascending b on one thread.  No float atomics: the same call gives the same bits.
// Gradient, fp32, contraction off:
//     s  = scale [* *scale_dev] [/ *norm_dev]  0, 1 or 2 roundings (as outreg.hip forms it)
//     qd = q_k0 + q_k1 + ..                    the entries of the frame with this pdf, ascending k
//     g' = fmaf(s, qd, g)                      ONE fma, then the rounding to nearest even of a 2-byte store
// A 2-BYTE GRADIENT IS THEREFORE ROUNDED TWICE: once by the call that stored it, once here.
//
// topk_rows_kernel: one four-wave workgroup per frame.  The row is read from memory ONCE into LDS as fp32 (rows of up to 9216
// elements; longer ones are re-read from memory in every round), then K rounds pick the next element in the order "value
// descending, index ascending" strictly behind the previous pick - nothing is marked, so the row in LDS is read-only -: every
// thread scans its elements, the wave reduces by the xor butterfly, the four waves through LDS (one barrier per round).  A NaN
// loses every comparison.  The normaliser is the fp32 sum of the picked values in slot order; the division is IEEE.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "../../include/pychain_hip.h"
#include "common.h"
#include "post.h"
#include "row_access.h"

namespace pychain_hip {
namespace {

constexpr int kPtNT = 256;                          // four waves

__device__ __forceinline__ float pt_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// XH: x's (and the gradient's) element type (one element at a time: row_load1, row_store1); GRAD: a gradient to update
template <int XH, bool GRAD>
__global__ __launch_bounds__(kPtNT) void post_frames_kernel(const PostArgs a, int nframes) {
  const int T = a.T, D = a.D, K = a.K;
  float s = 0.f;
  if constexpr (GRAD) {
#pragma clang fp contract(off)
    s = a.scale_dev ? a.scale * *a.scale_dev : a.scale;
    if (a.norm_dev) s = s / *a.norm_dev;
  }
  for (int f = blockIdx.x * kPtNT + threadIdx.x; f < nframes; f += gridDim.x * kPtNT) {
    const int b = f / T, t = f - b * T;
    if (t >= seq_len(a.lengths, b, T)) continue;              // padded frames: neither targets nor rows are read
    const int32_t* pd = a.pdfs + (size_t)f * K;
    const float* pr = a.probs + (size_t)f * K;
    const size_t row = (size_t)f * D;
    double acc = 0.0;
    int bad = 0;
    for (int k = 0; k < K; k++) {
      const int d = pd[k];
      if (d < 0) continue;                                    // padding
      if (d >= D) { bad++; continue; }
      const float q = pr[k];
      const double xd = (double)row_load1<XH>(a.x, row + d);
      const double c = xd < -30.0 ? -30.0 : (xd > 30.0 ? 30.0 : xd);
      acc = fma((double)q, c, acc);
      if constexpr (GRAD) {
        bool first = true;
        for (int j = 0; j < k; j++) first = first && pd[j] != d;
        if (first) {
          float qd = q;
          for (int j = k + 1; j < K; j++)
            if (pd[j] == d) qd = pt_add(qd, pr[j]);
          row_store1<XH>(a.grad, row + d, __builtin_fmaf(s, qd, row_load1<XH>(a.grad, row + d)));
        }
      }
    }
    a.frame_sums[f] = acc;
    a.frame_bad[f] = bad;
  }
}

// num_b = the sum of the live frames' values: fp64, fixed order (the pattern of outreg_seq_sum_kernel), rounded once
__global__ __launch_bounds__(kPtNT) void post_seq_sum_kernel(const double* frame_sums, const int32_t* frame_bad, const int64_t* lengths, int T,
                                                            double* seq_sums, int32_t* seq_bad, float* num_objf) {
  __shared__ double part[4];
  __shared__ int pbad[4];
  const int b = blockIdx.x, L = seq_len(lengths, b, T);
  const size_t base = (size_t)b * T;
  double acc = 0.0;
  int bad = 0;
  for (int t = threadIdx.x; t < L; t += kPtNT) { acc += frame_sums[base + t]; bad += frame_bad[base + t]; }
  acc = wave_sum_f64(acc);
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = acc; pbad[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = (part[0] + part[1]) + (part[2] + part[3]);
    seq_sums[b] = sum;
    seq_bad[b] = (pbad[0] + pbad[1]) + (pbad[2] + pbad[3]);
    num_objf[b] = (float)sum;
  }
}

// one thread, in stream order behind the denominator call that wrote `totals`
__global__ void post_totals_kernel(const double* seq_sums, const int32_t* seq_bad, int B, const float* den_objf, float loss_scale,
                                   const float* norm_dev, int32_t* bad_count, float* totals) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int bad = 0;
  for (int b = 0; b < B; b++) bad += seq_bad[b];
  *bad_count = bad;
  if (totals) {
    double sd = 0.0, sn = 0.0;
    for (int b = 0; b < B; b++) { sd += (double)den_objf[b]; sn += seq_sums[b]; }
    const double S = sd - sn;
    double v = (double)loss_scale * S;
    if (norm_dev) v /= (double)*norm_dev;
    const float full = (float)v;
    totals[0] = full; totals[4] = full;
    totals[3] = (float)S;
    totals[2] = totals[2] + (float)bad;
  }
}

// ---- top-k rows ---------------------------------------------------------------------------------------------------------------
// (v, i) is better than (bv, bi): value descending, index ascending; i == INT_MAX is "none"
__device__ __forceinline__ bool tk_better(float v, int i, float bv, int bi) {
  return i != INT_MAX && (bi == INT_MAX || v > bv || (v == bv && i < bi));
}

// XH: the rows' element type; VW: elements per load into LDS (1: rows whose base is not aligned, row_load1; 4 fp32 / 8 2-byte:
// written out here, the row goes to LDS in two float4 halves); CHIP: the row is held in LDS
template <int XH, int VW, bool CHIP>
__global__ __launch_bounds__(kPtNT) void topk_rows_kernel(const TopkArgs a, int dpad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  float* lrow = reinterpret_cast<float*>(tk_smem);                      // [dpad]
  float* part_v = lrow + dpad;                                          // [2][4]
  int* part_i = reinterpret_cast<int*>(part_v + 8);                     // [2][4]
  float* selv = reinterpret_cast<float*>(part_i + 8);                   // [kTopkMaxK]
  int* seli = reinterpret_cast<int*>(selv + kTopkMaxK);                 // [kTopkMaxK]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.T, D = a.D, K = a.K;
  const int f = blockIdx.x, b = f / T, t = f - b * T;
  int32_t* op = a.out_pdfs + (size_t)f * K;
  float* ov = a.out_probs + (size_t)f * K;
  if (t >= seq_len(a.lengths, b, T)) {                                  // padded frames: written, their rows never read
    if (tid < K) { op[tid] = -1; ov[tid] = 0.f; }
    return;
  }
  const size_t row = (size_t)f * D;
  if constexpr (CHIP) {
    for (int e = tid * VW; e < D; e += kPtNT * VW) {
      if constexpr (VW == 1) {
        lrow[e] = row_load1<XH>(a.rows, row + e);
      } else if constexpr (XH == kXF32) {
        *reinterpret_cast<float4*>(lrow + e) = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(a.rows) + row + e);
      } else {
        const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(a.rows) + row + e);
        float4 lo, hi;
        half2_to_f32(q.x, XH == kXBf16, lo.x, lo.y); half2_to_f32(q.y, XH == kXBf16, lo.z, lo.w);
        half2_to_f32(q.z, XH == kXBf16, hi.x, hi.y); half2_to_f32(q.w, XH == kXBf16, hi.z, hi.w);
        *reinterpret_cast<float4*>(lrow + e) = lo;
        *reinterpret_cast<float4*>(lrow + e + 4) = hi;
      }
    }
    __syncthreads();
  }
  const float floor = a.floor;
  float lastv = 0.f;
  int lasti = -1, n = 0;
  for (; n < K; n++) {
    float bv = 0.f;
    int bi = INT_MAX;
    for (int i = tid; i < D; i += kPtNT) {
      float v;
      if constexpr (CHIP) v = lrow[i];
      else v = row_load1<XH>(a.rows, row + i);
      // behind the previous pick in the order, at or above the floor (a NaN fails both), and above this thread's best so far
      const bool ok = v >= floor && (lasti < 0 || v < lastv || (v == lastv && i > lasti));
      if (ok && (bi == INT_MAX || v > bv)) { bv = v; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(bv, o);
      const int i2 = __shfl_xor(bi, o);
      if (tk_better(v2, i2, bv, bi)) { bv = v2; bi = i2; }
    }
    const int buf = (n & 1) * 4;
    if (lane == 0) { part_v[buf + wave] = bv; part_i[buf + wave] = bi; }
    __syncthreads();
    bv = part_v[buf]; bi = part_i[buf];
    for (int w = 1; w < 4; w++)
      if (tk_better(part_v[buf + w], part_i[buf + w], bv, bi)) { bv = part_v[buf + w]; bi = part_i[buf + w]; }
    if (bi == INT_MAX) break;                                           // (the same in every thread) nothing left at or above the floor
    if (tid == 0) { selv[n] = bv; seli[n] = bi; }
    lastv = bv; lasti = bi;
  }
  __syncthreads();
  if (tid < K) {
    if (tid < n) {
      float v = selv[tid];
      if (a.normalize) {
        float sum = 0.f;
        for (int j = 0; j < n; j++) sum = pt_add(sum, selv[j]);
        v = v / sum;
      }
      op[tid] = seli[tid]; ov[tid] = v;
    } else {
      op[tid] = -1; ov[tid] = 0.f;
    }
  }
}

template <int XH, bool GRAD>
void launch_frames_as(const PostArgs& a, int grid, int nframes, hipStream_t st) {
  hipLaunchKernelGGL((post_frames_kernel<XH, GRAD>), dim3(grid), dim3(kPtNT), 0, st, a, nframes);
}
template <int XH>
void launch_frames(const PostArgs& a, int grid, int nframes, hipStream_t st) {
  if (a.grad) launch_frames_as<XH, true>(a, grid, nframes, st);
  else launch_frames_as<XH, false>(a, grid, nframes, st);
}

template <int XH>
hipError_t launch_topk_as(const TopkArgs& a, int nframes, hipStream_t st) {
  constexpr int VW = XH == kXF32 ? 4 : 8;
  const size_t tail = sizeof(float) * (8 + 8 + 2 * kTopkMaxK);
  if (a.D > kTopkChipRow) {
    hipLaunchKernelGGL((topk_rows_kernel<XH, 1, false>), dim3(nframes), dim3(kPtNT), tail, st, a, 0);
  } else {
    const int dpad = (a.D + 7) / 8 * 8;
    const size_t lds = sizeof(float) * (size_t)dpad + tail;
    if (a.D % VW == 0 && ((uintptr_t)a.rows & 15) == 0)
      hipLaunchKernelGGL((topk_rows_kernel<XH, VW, true>), dim3(nframes), dim3(kPtNT), lds, st, a, dpad);
    else
      hipLaunchKernelGGL((topk_rows_kernel<XH, 1, true>), dim3(nframes), dim3(kPtNT), lds, st, a, dpad);
  }
  return hipGetLastError();
}

}  // namespace

size_t post_workspace_bytes(int B, int T) { return 12 * (size_t)B * T + 12 * (size_t)B + 32; }

hipError_t launch_post_frames(const PostArgs& a, hipStream_t st) {
  const size_t frames = (size_t)a.B * a.T;
  if (frames > (size_t)INT_MAX) return hipErrorInvalidValue;
  const int nframes = (int)frames, blocks = (nframes + kPtNT - 1) / kPtNT, grid = blocks < kRowPassMaxGrid ? blocks : kRowPassMaxGrid;
  if (a.x_half == kXF32) launch_frames<kXF32>(a, grid, nframes, st);
  else if (a.x_half == kXBf16) launch_frames<kXBf16>(a, grid, nframes, st);
  else launch_frames<kXF16>(a, grid, nframes, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(post_seq_sum_kernel, dim3(a.B), dim3(kPtNT), 0, st, a.frame_sums, a.frame_bad, a.lengths, a.T, a.seq_sums, a.seq_bad,
                     a.num_objf);
  return hipGetLastError();
}

hipError_t launch_post_totals(const double* seq_sums, const int32_t* seq_bad, int B, const float* den_objf, float loss_scale,
                              const float* norm_dev, int32_t* bad_count, float* totals, hipStream_t st) {
  hipLaunchKernelGGL(post_totals_kernel, dim3(1), dim3(1), 0, st, seq_sums, seq_bad, B, den_objf, loss_scale, norm_dev, bad_count, totals);
  return hipGetLastError();
}

hipError_t launch_topk_rows(const TopkArgs& a, hipStream_t st) {
  const size_t frames = (size_t)a.B * a.T;
  if (frames > (size_t)INT_MAX) return hipErrorInvalidValue;
  if (a.dtype == kXF32) return launch_topk_as<kXF32>(a, (int)frames, st);
  if (a.dtype == kXBf16) return launch_topk_as<kXBf16>(a, (int)frames, st);
  return launch_topk_as<kXF16>(a, (int)frames, st);
}

}  // namespace pychain_hip

using namespace pychain_hip;

// ---- the entry points (include/pychain_hip.h) -----------------------------------------------------------------------------------
extern "C" size_t pychain_hip_post_targets_workspace_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  return align256(post_workspace_bytes(B, T)) + 256;
}

extern "C" int pychain_hip_post_targets(
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, void* grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    const float* den_objf_per_seq, float* num_objf_per_seq, int32_t* bad_count,
    float loss_scale, float* totals, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "post_targets";
  if (nnet_output_dtype < PYCHAIN_HIP_F32 || nnet_output_dtype > PYCHAIN_HIP_F16)
    return fail(PYCHAIN_HIP_EINVAL, "%s: unknown nnet_output_dtype %d", who, nnet_output_dtype);
  if (!nnet_output || !seq_lengths || !target_pdfs || !target_probs || !num_objf_per_seq || !bad_count || !workspace)
    return fail(PYCHAIN_HIP_EINVAL, "%s: null pointer argument", who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  if (totals && !den_objf_per_seq) return fail(PYCHAIN_HIP_EINVAL, "%s: totals need den_objf_per_seq", who);
  if (((uintptr_t)grad | (uintptr_t)workspace) & 15) return fail(PYCHAIN_HIP_EINVAL, "%s: grad and workspace must be 16-byte aligned", who);
  const size_t need = pychain_hip_post_targets_workspace_bytes(B, T);
  if (workspace_bytes < need) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  const size_t BT = (size_t)B * T;
  PostArgs a;
  memset(&a, 0, sizeof(a));
  a.x = nnet_output; a.x_half = nnet_output_dtype; a.grad = grad; a.pdfs = target_pdfs; a.probs = target_probs; a.lengths = seq_lengths;
  a.scale = grad_scale; a.scale_dev = grad_scale_dev; a.norm_dev = loss_norm_dev;
  a.frame_sums = (double*)ws; a.seq_sums = (double*)(ws + 8 * BT);
  a.frame_bad = (int32_t*)(ws + 8 * BT + 8 * (size_t)B); a.seq_bad = a.frame_bad + BT;
  a.num_objf = num_objf_per_seq; a.B = B; a.T = T; a.D = D; a.K = K;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_post_frames(a, st);
  if (e == hipSuccess) e = launch_post_totals(a.seq_sums, a.seq_bad, B, den_objf_per_seq, loss_scale, loss_norm_dev, bad_count, totals, st);
  if (e != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "%s: %s", who, hipGetErrorString(e));
  return PYCHAIN_HIP_OK;
}

extern "C" int pychain_hip_topk_rows(const void* rows, int rows_dtype, const int64_t* seq_lengths, int B, int T, int D, int K, float floor,
                                     int normalize, int32_t* out_pdfs, float* out_probs, void* stream) {
  const char* who = "topk_rows";
  if (rows_dtype < PYCHAIN_HIP_F32 || rows_dtype > PYCHAIN_HIP_F16) return fail(PYCHAIN_HIP_EINVAL, "%s: unknown rows_dtype %d", who, rows_dtype);
  if (!rows || !seq_lengths || !out_pdfs || !out_probs) return fail(PYCHAIN_HIP_EINVAL, "%s: null pointer argument", who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1 || K > D || K > kTopkMaxK) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be in [1, min(D, %d)], got %d (D = %d)", who, kTopkMaxK, K, D);
  TopkArgs a;
  memset(&a, 0, sizeof(a));
  a.rows = rows; a.dtype = rows_dtype; a.lengths = seq_lengths; a.out_pdfs = out_pdfs; a.out_probs = out_probs; a.floor = floor;
  a.normalize = normalize; a.B = B; a.T = T; a.D = D; a.K = K;
  hipError_t e = launch_topk_rows(a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "%s: %s", who, hipGetErrorString(e));
  return PYCHAIN_HIP_OK;
}
