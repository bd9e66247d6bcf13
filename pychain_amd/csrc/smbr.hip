// smbr.hip - lattice-free sMBR (include/pychain_hip.h: pychain_hip_smbr_*): the expected frame accuracy of the
// denominator's path distribution against a reference given as sparse per-frame targets, E = sum_t sum_n gamma(t,n) A(t,n), and
// its gradient dE/dy(t,n) = gamma(t,n) (E[score | pdf n at t] - E).  The gradient is a covariance under the path distribution:
// beside alpha' and beta' it needs the accuracy-weighted pair alpha-bar', beta-bar', which no other kernel of the library forms.
//
//   smbr_frame_acc_kernel    e(b,t) = sum_k q_k gamma(b,t,pdf_k) from the occupancies of the ordinary denominator call, and
//                            E_b = sum_t e(b,t) in fp64.  One workgroup per sequence, a thread per frame.
//   smbr_recursion_kernel    2B persistent workgroups, one per (sequence, direction), each carrying (alpha', alpha-bar') or
//                            (beta', beta-bar') in LDS, double-buffered, with the frame's row x = exp(clamp(y)) and its sparse
//                            companion xa(n) = x(n) A(t,n); both rows are made a frame ahead.  Arcs come from global memory in the
//                            reference layout (by destination forwards, by source backwards); a thread owns states tid, tid + 1024,
//                            ...  The accuracies are CENTRED, a(t,n) = A(t,n) - e(t): the source term of a frame is
//                            sum alpha' p xa - e(t) * (the first-order sum), so that only the frame's K entries need a row.
//                            alpha-bar and beta-bar take the per-frame normalisers of alpha and beta.  No workgroup waits for
//                            another; every loop is bounded by L_b <= T.
//   smbr_grad_kernel         time-parallel over (sequence, block of frames): the four state rows of a frame in LDS, a thread owns
//                            pdfs tid, tid + 512, ... and walks that pdf's arcs through the caller's by-pdf order:
//                              q0 = sum p alpha' beta',  q1 = sum p (alpha-bar' beta' + alpha' beta-bar')
//                              v = x (q1 + a q0),  grad = s (v - eps x q0) / sum_m x(m) q0(m),  eps = sum_m v(m) / sum_m x(m) q0(m)
//                            (the row centred by its own mean: §3.26, "the residue")
//                            The frame's normalisers cancel in the quotient, as in den_general_gamma_kernel.
//
// The same with the accuracy by CLASS (pychain_hip_smbr_*_classes): A(t,n) = Acls(t, cls[n]) for a map cls from
// pdf to class, Acls(t,c) = the sum of the frame's q_k whose class is c.  A row of A is dense then, which none of the three
// kernels above can take, so each has a counterpart; the pdf-level kernels keep their code.
//   smbr_class_frame_acc_kernel   a dense pass over gamma: a wave per frame on a grid over (frames, B), the frame's entries merged
//                                 into distinct classes first, fp64 sums in a fixed order; smbr_class_seq_acc_kernel sums E_b
//   smbr_class_recursion_kernel   the recursion with CLS: one table Acls(t, .) in LDS, written for the next frame before the arc
//                                 loop; the dense companion row x A is made behind the reduction's barrier, where the pdf-level
//                                 form scatters its K entries.  No barrier more, the arc loop unchanged.
//   smbr_class_grad_kernel        the frame's table made beside the state rows; every carried pdf takes its class's credit; the
//                                 row is centred by its own mean (the residue of e(t)'s rounding, which a dense A would spread)
// Nothing is atomic but integer counters and flags; every sum has a fixed order, so a call gives the same bits every time.  All of
// this unit's device code, the helpers of the project's headers included, is compiled with contraction off: the 2-byte forms then compute what the fp32 form computes on the up-cast input.
//
// These kernels keep a frame in LDS and the two entry points that launch only them refuse what does not fit.  The general kernels
// (smbr_general.hip) take any graph and tree with the same bits; they share this unit's argument checks, workspace
// layout and entry-point code (pychain_hip_smbr_forward_backward_general, pychain_hip_smbr_form, below).
// The bodies of the four stage-2 kernels are not here: `recursion`, `smbr_grad_frame` and `smbr_close` of smbr_device.h are shared
// with the general kernels and with the expected arc counts (arc_counts.hip); the kernels below lay out their LDS and instantiate
// them over FrameLds.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#pragma clang fp contract(off)      // ahead of the project's headers: their inline helpers (clamp_exp, the row loads) are under it too

#include "../../include/pychain_hip.h"
#include "call_args.h"
#include "common.h"
#include "row_access.h"
#include "smbr.h"
#include "smbr_device.h"

namespace pychain_hip {
namespace {

// (the workgroup shapes, the helpers and the bodies of stage 2: smbr_device.h)
constexpr int kSmAccNT = 256;

// ---- stage 1: frame accuracies ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSmAccNT) void smbr_frame_acc_kernel(const SmbrAccArgs a) {
  __shared__ double red[kSmAccNT / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int L = seq_len(a.lengths, b, a.T);
  double sum = 0.0;
  int bad = 0;
  for (int t = tid; t < L; t += kSmAccNT) {
    const size_t f = (size_t)b * a.T + t;
    const float* g = a.gamma + f * a.D;
    double e = 0.0;
    for (int k = 0; k < a.Kt; k++) {
      const int d = a.pdfs[f * a.Kt + k];
      if (d < 0) continue;
      if (d >= a.D) { bad++; continue; }
      e += (double)a.probs[f * a.Kt + k] * (double)g[d];
    }
    a.frame_acc[f] = (float)e;
    sum += e;
  }
  sum = wave_sum_f64(sum);
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((tid & 63) == 0) {
    red[tid >> 6] = sum;
    if (bad) atomicAdd(a.bad_count + 1, bad);                 // (an integer sum: the same value in any order)
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < kSmAccNT / 64; w++) s += red[w];
    a.acc_per_seq[b] = s;
  }
}

// The same by class: e(b,t) = sum_n gamma(b,t,n) Acls(t, cls[n]) is a dense pass over gamma, so a wave takes a frame on a grid over
// (frames, B) - kSmAccWaves frames a workgroup, no barrier.  The frame's entries are merged first: lane k keeps (class, summed q)
// of entry k where its class occurs first in the frame, q summed in ascending k (entries beyond 64: in chunks of a wave).  Every
// lane then walks its elements in ascending n against the merged entries, read lane by lane; the products are summed in fp64 per
// lane and over the wave by the butterfly.  E_b is summed from the fp64 frame values by a launch of its own.
constexpr int kSmAccWaves = kSmAccNT / 64;
template <int VW>
__global__ __launch_bounds__(kSmAccNT) void smbr_class_frame_acc_kernel(const SmbrAccArgs a, const SmbrClasses c) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int t = blockIdx.x * kSmAccWaves + (threadIdx.x >> 6);
  if (t >= seq_len(a.lengths, b, a.T)) return;                                 // (the whole wave)
  const size_t f = (size_t)b * a.T + t;
  const int32_t* pd = a.pdfs + f * a.Kt;
  const float* pr = a.probs + f * a.Kt;
  const float* g = a.gamma + f * a.D;
  const int D = a.D, Kt = a.Kt;
  double e = 0.0;
  int bad = 0;
  for (int k0 = 0; k0 < Kt; k0 += 64) {
    const int k = k0 + lane;
    int mc = -1;
    float mq = 0.f;
    if (k < Kt) {
      if (pd[k] >= (c.targets_are_classes ? c.C : D)) bad++;
      mc = entry_class(c, pd[k], D);
      for (int j = 0; j < k && mc >= 0; j++)
        if (entry_class(c, pd[j], D) == mc) mc = -1;
      if (mc >= 0) {
        mq = pr[k];
        for (int j = k + 1; j < Kt; j++)
          if (entry_class(c, pd[j], D) == mc) mq += pr[j];
      }
    }
    const int live = min(64, Kt - k0);
    for (int base = 0; base < D; base += 64 * VW) {                            // (the same trips in every lane: the lane reads below)
      const int n0 = base + lane * VW;
      float v[VW], av[VW];
      int cn[VW];
#pragma unroll
      for (int i = 0; i < VW; i++) { v[i] = 0.f; av[i] = 0.f; cn[i] = -2; }
      if (n0 < D) {
        row_load<kXF32, VW>(g, (size_t)n0, v);
        if constexpr (VW == 4) {
          const int4 q = *reinterpret_cast<const int4*>(c.cls + n0);
          cn[0] = q.x; cn[1] = q.y; cn[2] = q.z; cn[3] = q.w;
        } else {
          cn[0] = c.cls[n0];
        }
      }
      for (int j = 0; j < live; j++) {
        const int jc = __builtin_amdgcn_readlane(mc, j);
        const float jq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mq), j));
#pragma unroll
        for (int i = 0; i < VW; i++)
          if (cn[i] == jc) av[i] = jq;                                         // (at most one merged entry has the class)
      }
#pragma unroll
      for (int i = 0; i < VW; i++) e += (double)v[i] * (double)av[i];
    }
  }
  e = wave_sum_f64(e);
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if (lane == 0) {
    a.frame_acc[f] = (float)e;
    c.frame_e[f] = e;
    if (bad) atomicAdd(a.bad_count + 1, bad);                                  // (an integer sum: the same value in any order)
  }
}
// E_b = sum_t e(b,t) in fp64: one workgroup per sequence, a thread per frame, the order of smbr_frame_acc_kernel
__global__ __launch_bounds__(kSmAccNT) void smbr_class_seq_acc_kernel(const SmbrAccArgs a, const SmbrClasses c) {
  __shared__ double red[kSmAccNT / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int L = seq_len(a.lengths, b, a.T);
  double sum = 0.0;
  for (int t = tid; t < L; t += kSmAccNT) sum += c.frame_e[(size_t)b * a.T + t];
  sum = wave_sum_f64(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < kSmAccNT / 64; w++) s += red[w];
    a.acc_per_seq[b] = s;
  }
}

// ---- stage 2: the recursions ----------------------------------------------------------------------------------------------------
// the body: smbr_device.h, `recursion` with the weighted pair over FrameLds.  LDS: [2][H] alpha' / beta', [2][H] alpha-bar' /
// beta-bar', [2][D] x, [2][D] x A, the reduction scratch and, by class, the table [C]
template <int XH, bool CLS>
__device__ __forceinline__ void smbr_recursion(const SmbrArgs& a, const SmbrClasses& c) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  const size_t H = a.g.H, D = a.D;
  RecArgs r = smbr_rec_args(a);
  r.vec0 = lds; r.vec1 = r.vec0 + 2 * H; r.xrow = r.vec1 + 2 * H; r.xacc = r.xrow + 2 * D; r.red = r.xacc + 2 * D; r.acl = r.red + kSmRed;
  if (blockIdx.x < (unsigned)a.B) recursion<XH, true, CLS, true, FrameLds>(r, c, blockIdx.x);
  else recursion<XH, false, CLS, true, FrameLds>(r, c, blockIdx.x - a.B);
}
template <int XH>
__global__ __launch_bounds__(kSmNT) void smbr_recursion_kernel(const SmbrArgs a) {
  smbr_recursion<XH, false>(a, SmbrClasses{});
}
template <int XH>
__global__ __launch_bounds__(kSmNT) void smbr_class_recursion_kernel(const SmbrArgs a, const SmbrClasses c) {
  smbr_recursion<XH, true>(a, c);
}

// ---- stage 2: the gradient ------------------------------------------------------------------------------------------------------
// the frame: smbr_device.h, smbr_grad_frame over FrameLds.  LDS: the four state rows [4][H], [D] x q0, [D] x (q1 + a q0), the
// reduction scratch and, by class, the frame's table [C].  The sequence's first workgroup closes it.
template <int XH, bool CLS>
__device__ __forceinline__ void smbr_grad(const SmbrArgs& a, const SmbrClasses& c) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lds = reinterpret_cast<float*>(smem_raw);
  const int b = blockIdx.y, H = a.g.H, D = a.D;
  const int L = seq_len(a.lengths, b, a.T);
  float* const gq = lds + 4 * (size_t)H;
  float* const gv = gq + D;
  float* const red = gv + D;
  const float gscale = a.grad_scale_dev ? a.grad_scale * *a.grad_scale_dev : a.grad_scale;
  const int t_begin = blockIdx.x * kSmFrames, t_end = min(t_begin + kSmFrames, a.T);
  for (int t = t_begin; t < t_end; t++) smbr_grad_frame<XH, CLS, FrameLds>(a, c, b, t, L, gscale, lds, gq, gv, red + kSmRed, red);
  if (blockIdx.x == 0) smbr_close(a, b, L, red);
}
template <int XH>
__global__ __launch_bounds__(kSmGNT) void smbr_grad_kernel(const SmbrArgs a) {
  smbr_grad<XH, false>(a, SmbrClasses{});
}
template <int XH>
__global__ __launch_bounds__(kSmGNT) void smbr_class_grad_kernel(const SmbrArgs a, const SmbrClasses c) {
  smbr_grad<XH, true>(a, c);
}

// the recursion launch, then the gradient launch; c.cls null: the pdf-level kernels
template <int XH>
hipError_t launch_as(const SmbrArgs& a, const SmbrClasses& c, hipStream_t st) {
  const size_t lds_r = smbr_recursion_lds(a.g.H, a.D, c.C), lds_g = smbr_grad_lds(a.g.H, a.D, c.C);
  const dim3 grid_r(2 * a.B), grid_g((a.T + kSmFrames - 1) / kSmFrames, a.B);
  hipError_t e = c.cls ? launch_with_lds(smbr_class_recursion_kernel<XH>, grid_r, dim3(kSmNT), lds_r, st, a, c)
                       : launch_with_lds(smbr_recursion_kernel<XH>, grid_r, dim3(kSmNT), lds_r, st, a);
  if (e != hipSuccess) return e;
  return c.cls ? launch_with_lds(smbr_class_grad_kernel<XH>, grid_g, dim3(kSmGNT), lds_g, st, a, c)
               : launch_with_lds(smbr_grad_kernel<XH>, grid_g, dim3(kSmGNT), lds_g, st, a);
}

}  // namespace

size_t smbr_recursion_lds(int H, int D) { return (4 * (size_t)H + 4 * (size_t)D + kSmRed) * sizeof(float); }
size_t smbr_grad_lds(int H, int D) { return (4 * (size_t)H + 2 * (size_t)D + kSmRed) * sizeof(float); }
size_t smbr_recursion_lds(int H, int D, int C) { return smbr_recursion_lds(H, D) + (size_t)C * sizeof(float); }
size_t smbr_grad_lds(int H, int D, int C) { return smbr_grad_lds(H, D) + (size_t)C * sizeof(float); }
size_t smbr_lds_bytes(int H, int D, int C) {       // (the gradient kernel has no static LDS, and fewer rows)
  const size_t r = smbr_recursion_lds(H, D, C) + kSmStaticLds, g = smbr_grad_lds(H, D, C);
  return r > g ? r : g;
}

hipError_t launch_smbr_frame_acc(const SmbrAccArgs& a, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.bad_count, 0, 2 * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(smbr_frame_acc_kernel, dim3(a.B), dim3(kSmAccNT), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_smbr_frame_acc(const SmbrAccArgs& a, const SmbrClasses& c, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.bad_count, 0, 2 * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  const dim3 grid((a.T + kSmAccWaves - 1) / kSmAccWaves, a.B);
  // float4 / int4 loads where every row of gamma and the map start on the 16-byte grid, else one element at a time
  const bool wide = a.D % 4 == 0 && ((uintptr_t)a.gamma | (uintptr_t)c.cls) % 16 == 0;
  if (wide) hipLaunchKernelGGL(smbr_class_frame_acc_kernel<4>, grid, dim3(kSmAccNT), 0, st, a, c);
  else hipLaunchKernelGGL(smbr_class_frame_acc_kernel<1>, grid, dim3(kSmAccNT), 0, st, a, c);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(smbr_class_seq_acc_kernel, dim3(a.B), dim3(kSmAccNT), 0, st, a, c);
  return hipGetLastError();
}

hipError_t launch_smbr(const SmbrArgs& a, const SmbrClasses& c, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(a.seq_bad, 0, 2 * (size_t)a.B * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  return by_row_dtype(a.x_half, [&](auto xh) { return launch_as<decltype(xh)::value>(a, c, st); });
}

}  // namespace pychain_hip

using namespace pychain_hip;

// ---- the entry points (include/pychain_hip.h) -----------------------------------------------------------------------------------
namespace {
struct SmbrCarve { size_t al, ab, be, bb, tot_a, tot_b, seq_bad, end, total; };
SmbrCarve smbr_carve(int B, int T, int H) {
  SmbrCarve c;
  const size_t traj = align256((size_t)B * (T + 1) * H * sizeof(float)), tot = align256((size_t)B * (T + 1) * sizeof(float));
  size_t o = 0;
  c.al = o; o += traj; c.ab = o; o += traj; c.be = o; o += traj; c.bb = o; o += traj;
  c.tot_a = o; o += tot; c.tot_b = o; o += tot;
  c.seq_bad = o; o += align256(2 * (size_t)B * sizeof(int32_t));
  c.end = o;
  c.total = o + 256;                               // (the base is aligned inside the caller's buffer)
  return c;
}
// the general kernels' scratch rows (smbr.h: SmbrGeneral) behind the layout above, which they keep
struct SmbrGeneralCarve { size_t rec, grad, total; SmbrGeneral s; };
SmbrGeneralCarve smbr_general_carve(const SmbrCarve& c, int B, int T, int D, int C) {
  SmbrGeneralCarve v;
  memset(&v, 0, sizeof(v));
  v.s.rec_stride = smbr_general_rec_stride(D, C);
  v.s.grad_stride = smbr_general_grad_stride(D, C);
  v.s.grad_wgs = smbr_general_grad_wgs(B, T);
  size_t o = c.end;
  v.rec = o; o += align256(2 * (size_t)B * v.s.rec_stride * sizeof(float));
  v.grad = o; o += align256((size_t)v.s.grad_wgs * v.s.grad_stride * sizeof(float));
  v.total = o + 256;
  return v;
}

// The form a call of the general entry point runs (include/pychain_hip.h: PYCHAIN_HIP_SMBR_*), or a negative code with the
// message set.  C = 0: the pdf-level call.
int smbr_resolve_form(const char* who, int H, int D, int C, int requested) {
  if (H <= 0 || D <= 0 || C < 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes H=%d D=%d num_classes=%d", who, H, D, C);
  if (requested < PYCHAIN_HIP_SMBR_AUTO || requested > PYCHAIN_HIP_SMBR_GLOBAL)
    return fail(PYCHAIN_HIP_EINVAL, "%s: unknown form %d (PYCHAIN_HIP_SMBR_AUTO .. _GLOBAL)", who, requested);
  const size_t lds = smbr_lds_bytes(H, D, C), rows = smbr_general_lds(H);
  if (requested == PYCHAIN_HIP_SMBR_LDS && lds > kSmbrLdsBudget)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: the LDS form needs %zu bytes of LDS for %d states, %d pdfs and %d classes (four state vectors, four rows and the class table), a CU has %zu",
                who, lds, H, D, C, kSmbrLdsBudget);
  if (requested == PYCHAIN_HIP_SMBR_ROWS && rows > kSmbrLdsBudget)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: the rows form needs %zu bytes of LDS for %d states (four state vectors), a CU has %zu",
                who, rows, H, kSmbrLdsBudget);
  if (requested != PYCHAIN_HIP_SMBR_AUTO) return requested;
  return lds <= kSmbrLdsBudget ? PYCHAIN_HIP_SMBR_LDS : rows <= kSmbrLdsBudget ? PYCHAIN_HIP_SMBR_ROWS : PYCHAIN_HIP_SMBR_GLOBAL;
}
constexpr int kSmbrFormOfOld = -1;                 // the two entry points from before the general kernels: LDS or refused, their messages
}  // namespace

extern "C" int pychain_hip_smbr_form(int H, int D, int num_classes, int requested) {
  return smbr_resolve_form("smbr_form", H, D, num_classes, requested);
}

extern "C" size_t pychain_hip_smbr_general_lds_bytes(int H) {
  if (H <= 0) return 0;
  return smbr_general_lds(H);
}

extern "C" size_t pychain_hip_smbr_general_workspace_bytes(int B, int T, int H, int D, int num_classes) {
  if (B <= 0 || T <= 0 || H <= 0 || D <= 0 || num_classes < 0) return 0;
  return smbr_general_carve(smbr_carve(B, T, H), B, T, D, num_classes).total;
}

extern "C" size_t pychain_hip_smbr_workspace_bytes(int B, int T, int H) {
  if (B <= 0 || T <= 0 || H <= 0) return 0;
  return smbr_carve(B, T, H).total;
}

extern "C" size_t pychain_hip_smbr_frame_accuracy_classes_workspace_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  return align256((size_t)B * T * sizeof(double)) + 256;
}

extern "C" size_t pychain_hip_smbr_lds_bytes(int H, int D, int num_classes) {
  if (H <= 0 || D <= 0 || num_classes < 0) return 0;
  return smbr_lds_bytes(H, D, num_classes);
}

namespace {
// what a class call says of its map: `cls` is the caller's, non-null
int bad_classes(const char* who, int num_classes) {
  if (num_classes < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: num_classes must be at least 1 with pdf_classes, got %d", who, num_classes);
  return PYCHAIN_HIP_OK;
}
int classes_without_map(const char* who) {
  return fail(PYCHAIN_HIP_EINVAL, "%s: targets_are_classes needs pdf_classes", who);
}

// both accuracy entry points; `pdf_classes` null: the pdf-level launch
int smbr_frame_accuracy(const char* who, const float* gamma, const int64_t* seq_lengths, int B, int T, int D,
                        const int32_t* target_pdfs, const float* target_probs, int K,
                        float* frame_acc, double* acc_per_seq, int32_t* bad_count, void* stream,
                        const int32_t* pdf_classes, int num_classes, int targets_are_classes, void* workspace, size_t workspace_bytes) {
  if (!gamma || !seq_lengths || !target_pdfs || !target_probs || !frame_acc || !acc_per_seq || !bad_count) return null_pointer(who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  if ((size_t)B * T > (size_t)INT_MAX) return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: B * T = %zu frames", who, (size_t)B * T);
  SmbrAccArgs a;
  memset(&a, 0, sizeof(a));
  a.gamma = gamma; a.lengths = seq_lengths; a.pdfs = target_pdfs; a.probs = target_probs; a.frame_acc = frame_acc;
  a.acc_per_seq = acc_per_seq; a.bad_count = bad_count; a.B = B; a.T = T; a.D = D; a.Kt = K;
  hipError_t err;
  if (pdf_classes) {
    const int rc = bad_classes(who, num_classes);
    if (rc != PYCHAIN_HIP_OK) return rc;
    if (!workspace) return null_pointer(who);
    const size_t need = pychain_hip_smbr_frame_accuracy_classes_workspace_bytes(B, T);
    if (workspace_bytes < need) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    const SmbrClasses c{pdf_classes, num_classes, targets_are_classes != 0, (double*)ws_base(workspace)};
    err = launch_smbr_frame_acc(a, c, (hipStream_t)stream);
  } else {
    err = launch_smbr_frame_acc(a, (hipStream_t)stream);
  }
  if (err != hipSuccess) return launch_failed(who, err, nullptr);
  return PYCHAIN_HIP_OK;
}
}  // namespace

extern "C" int pychain_hip_smbr_frame_accuracy(const float* gamma, const int64_t* seq_lengths, int B, int T, int D,
                                               const int32_t* target_pdfs, const float* target_probs, int K,
                                               float* frame_acc, double* acc_per_seq, int32_t* bad_count, void* stream) {
  return smbr_frame_accuracy("smbr_frame_accuracy", gamma, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc, acc_per_seq, bad_count,
                             stream, nullptr, 0, 0, nullptr, 0);
}

extern "C" int pychain_hip_smbr_frame_accuracy_classes(const float* gamma, const int64_t* seq_lengths, int B, int T, int D,
                                                       const int32_t* target_pdfs, const float* target_probs, int K,
                                                       float* frame_acc, double* acc_per_seq, int32_t* bad_count, void* stream,
                                                       const int32_t* pdf_classes, int num_classes, int targets_are_classes,
                                                       void* workspace, size_t workspace_bytes) {
  if (!pdf_classes) {                              // the pdf-level call, launch for launch
    if (targets_are_classes) return classes_without_map("smbr_frame_accuracy_classes");
    return pychain_hip_smbr_frame_accuracy(gamma, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc, acc_per_seq, bad_count, stream);
  }
  return smbr_frame_accuracy("smbr_frame_accuracy_classes", gamma, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc, acc_per_seq,
                             bad_count, stream, pdf_classes, num_classes, targets_are_classes, workspace, workspace_bytes);
}

namespace {
// both recursion entry points; `pdf_classes` null: the pdf-level launches
int smbr_forward_backward(
    const char* who,
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes, int form) {
  const NumGraphs graphs{ft, fi, fp, bt, bi, bp, initial, final_, 0, H, num_arcs};
  const Rows rows{nnet_output, nnet_output_dtype, seq_lengths, B, T, D};
  int rc = bad_dtype(who, nnet_output_dtype);
  if (rc != PYCHAIN_HIP_OK) return rc;
  if (graphs.any_null() || !leaky || !pdf_arcs || !pdf_index || !rows.x || !rows.lengths || !target_pdfs || !target_probs || !frame_acc ||
      !grad || !acc_per_seq || !closing || !bad_count || !workspace)
    return null_pointer(who);
  if ((rc = bad_sizes(who, rows, graphs)) != PYCHAIN_HIP_OK) return rc;
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  if (!(leaky_hmm_coefficient > 0.f && leaky_hmm_coefficient < 1.f))
    return fail(PYCHAIN_HIP_EINVAL, "%s: leaky_hmm_coefficient must be in (0,1), got %g", who, (double)leaky_hmm_coefficient);
  if (pdf_classes && (rc = bad_classes(who, num_classes)) != PYCHAIN_HIP_OK) return rc;
  const int C = pdf_classes ? num_classes : 0;
  int run = PYCHAIN_HIP_SMBR_LDS;
  if (form == kSmbrFormOfOld) {
    if (pdf_classes) {
      const size_t need = smbr_lds_bytes(H, D, num_classes);
      if (need > kSmbrLdsBudget)
        return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: %d states, %d pdfs and %d classes need %zu bytes of LDS (four state vectors, four rows and the class table), a CU has %zu",
                    who, H, D, num_classes, need, kSmbrLdsBudget);
    }
    const size_t lds = smbr_recursion_lds(H, D);
    if (!pdf_classes && lds + kSmStaticLds > kSmbrLdsBudget)
      return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: %d states and %d pdfs need %zu bytes of LDS (four state vectors and four rows), a CU has %zu",
                  who, H, D, lds + kSmStaticLds, kSmbrLdsBudget);
  } else if ((run = smbr_resolve_form(who, H, D, C, form)) < 0) {
    return run;
  }
  if ((size_t)B * (T + 1) > (size_t)INT_MAX) return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: B * (T + 1) = %zu rows", who, (size_t)B * (T + 1));
  const SmbrCarve c = smbr_carve(B, T, H);
  SmbrGeneralCarve gc = smbr_general_carve(c, B, T, D, C);
  const size_t ws_need = run == PYCHAIN_HIP_SMBR_LDS ? c.total : gc.total;     // (the LDS form takes the trajectories alone)
  if (workspace_bytes < ws_need) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, ws_need);
  char* base = ws_base(workspace);
  SmbrArgs a;
  memset(&a, 0, sizeof(a));
  a.g = SmbrGraph{ft, fi, fp, bt, bi, bp, leaky, initial, final_, pdf_arcs, pdf_index, H, num_arcs};
  a.x = nnet_output; a.x_half = nnet_output_dtype; a.lengths = seq_lengths; a.pdfs = target_pdfs; a.probs = target_probs;
  a.frame_acc = frame_acc; a.coef = leaky_hmm_coefficient; a.grad_scale = grad_scale; a.grad_scale_dev = grad_scale_dev;
  a.grad = grad; a.acc_per_seq = acc_per_seq; a.closing = closing; a.bad_count = bad_count;
  a.al = (float*)(base + c.al); a.ab = (float*)(base + c.ab); a.be = (float*)(base + c.be); a.bb = (float*)(base + c.bb);
  a.tot_a = (float*)(base + c.tot_a); a.tot_b = (float*)(base + c.tot_b); a.seq_bad = (int32_t*)(base + c.seq_bad);
  a.B = B; a.T = T; a.D = D; a.Kt = K;
  const SmbrClasses cl{pdf_classes, C, targets_are_classes != 0, nullptr};
  hipError_t err;
  if (run == PYCHAIN_HIP_SMBR_LDS) {
    err = launch_smbr(a, cl, (hipStream_t)stream);
  } else {
    gc.s.rec = (float*)(base + gc.rec); gc.s.grad = (float*)(base + gc.grad);
    gc.s.state_lds = run == PYCHAIN_HIP_SMBR_ROWS;
    err = launch_smbr_general(a, cl, gc.s, (hipStream_t)stream);
  }
  if (err != hipSuccess) return launch_failed(who, err, nullptr);
  return PYCHAIN_HIP_OK;
}
}  // namespace

extern "C" int pychain_hip_smbr_forward_backward(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream) {
  return smbr_forward_backward("smbr_forward_backward", ft, fi, fp, bt, bi, bp, leaky, initial, final_, pdf_arcs, pdf_index, H, num_arcs,
                               nnet_output, nnet_output_dtype, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc,
                               leaky_hmm_coefficient, grad_scale, grad_scale_dev, grad, acc_per_seq, closing, bad_count,
                               workspace, workspace_bytes, stream, nullptr, 0, 0, kSmbrFormOfOld);
}

extern "C" int pychain_hip_smbr_forward_backward_classes(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes) {
  if (!pdf_classes && targets_are_classes) return classes_without_map("smbr_forward_backward_classes");
  return smbr_forward_backward(pdf_classes ? "smbr_forward_backward_classes" : "smbr_forward_backward", ft, fi, fp, bt, bi, bp, leaky, initial,
                               final_, pdf_arcs, pdf_index, H, num_arcs, nnet_output, nnet_output_dtype, seq_lengths, B, T, D, target_pdfs,
                               target_probs, K, frame_acc, leaky_hmm_coefficient, grad_scale, grad_scale_dev, grad, acc_per_seq, closing,
                               bad_count, workspace, workspace_bytes, stream, pdf_classes, num_classes, targets_are_classes, kSmbrFormOfOld);
}

// any H, num_pdfs, num_classes: `form` picks the kernels, PYCHAIN_HIP_SMBR_LDS today's launches
extern "C" int pychain_hip_smbr_forward_backward_general(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes, int form) {
  if (!pdf_classes && targets_are_classes) return classes_without_map("smbr_forward_backward_general");
  if (form < PYCHAIN_HIP_SMBR_AUTO || form > PYCHAIN_HIP_SMBR_GLOBAL)
    return fail(PYCHAIN_HIP_EINVAL, "smbr_forward_backward_general: unknown form %d (PYCHAIN_HIP_SMBR_AUTO .. _GLOBAL)", form);
  return smbr_forward_backward("smbr_forward_backward_general", ft, fi, fp, bt, bi, bp, leaky, initial, final_, pdf_arcs, pdf_index, H, num_arcs,
                               nnet_output, nnet_output_dtype, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc,
                               leaky_hmm_coefficient, grad_scale, grad_scale_dev, grad, acc_per_seq, closing, bad_count,
                               workspace, workspace_bytes, stream, pdf_classes, num_classes, targets_are_classes, form);
}
