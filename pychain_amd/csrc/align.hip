// align.hip - Viterbi (best-path) alignment over log-domain numerator graphs for gfx950: the max-plus sibling of the
// numerator's forward pass (num_kernels.hip: num_fb_kernel), followed by a backtrace.
//
//   align_kernel           B persistent workgroups, one per sequence.  Forward: one state per thread, the sequence's arcs by
//                          destination in LDS, fp64 ping-pong score vectors, row-staging waves, ONE barrier per frame; per
//                          frame every state writes the offset of its winning arc inside its [lo, hi) as a uint16
//                          backpointer row (2 H bytes, coalesced).  Then a workgroup argmax over s(L,.) + final and the
//                          backtrace in the same workgroup: blocks of backpointer rows are read back by all but the first
//                          wave, turned into the winning arc's packed (state, pdf) and staged in LDS, while one lane walks the
//                          previous block inside LDS (one dependent LDS read per frame) - double-buffered, one barrier per block.
//   align_general_kernel   graphs beyond the tile kernels (num_needs_general): score vectors and int32 backpointers in the
//                          workspace, states strided over 1024 threads, a barrier per frame, a plain walk at the end.  It
//                          reads the time windows from global memory where they are.
//
// Both reach the same bits as the host twin (cpu.cpp: align_one): fp64 adds and compares only, in the association
//   s(t+1,h) = max_k  s(t,src_k) + ((double)lp_k + (double)clamp(x(t,pdf_k)))      (first k in list order wins ties)
//   score    = max_h  s(L,h) + (double)final(h)                                      (lowest h wins ties)
// TW: alignment time windows (AlignArgs::windows, include/pychain_hip.h: pychain_hip_align_tw): a state outside its window at
// time t gets -inf and backpointer 0 and skips its arcs - the select after the max, and a NaN term that reaches only masked
// states goes no further; the initial row and the final argmax take the mask.  A flag of the template, as num_fb_kernel's: the
// instantiations without it keep their instructions.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pychain_hip.h"
#include "call_args.h"
#include "common.h"
#include "device_utils.h"
#include "num_kernels.h"

namespace pychain_hip {

// (outside the unnamed namespace: the kernel symbols carry its name)
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

namespace {

constexpr int kAlNT = 512;                 // threads that own states (one state per thread up to 512 states)
constexpr int kAlLd = 128;                 // row-staging threads (num_kernels.hip: kFbLd)
constexpr int kAlPre = 24;                 // backpointers a converting thread holds in registers per block
constexpr int kAlWalkCap = 96 * 1024;      // LDS the backtrace stages rows in, at most (more where the forward's buffers are larger)
constexpr int kAlGT = 1024;                // align_general_kernel

struct AArc { uint32_t pk; float lp; };    // pk = src | pdf << 16

__device__ __forceinline__ double canonical_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// a word written by another thread of this workgroup before the last barrier: read around the vector L1 (num_general.hip: fresh)
__device__ __forceinline__ uint32_t fresh_u32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t fresh_i32(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double fresh_f64(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// torch.clamp(x, -30, 30) keeps a NaN (pychain/loss.py:30): so does this
__device__ __forceinline__ float aclamp(float x) { return x != x ? x : fminf(fmaxf(x, -30.f), 30.f); }

// (value, index) with the larger value; equal values: the lower index.  NaN never enters (the callers skip it).
__device__ __forceinline__ void argmax_merge(double& v, int& i, double ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void wave_argmax(double& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    argmax_merge(v, i, ov, oi);
  }
}

// -1 into every row of sequence b the path does not cover (all of them where there is no path)
__device__ __forceinline__ void pad_rows(const AlignArgs& a, int b, int L, bool ok, int tid, int nt) {
  int64_t* pd = a.pdfs + (size_t)b * a.T;
  int32_t* st = a.states + (size_t)b * (a.T + 1);
  for (int t = (ok ? L : 0) + tid; t < a.T; t += nt) pd[t] = -1;
  for (int t = (ok ? L + 1 : 0) + tid; t <= a.T; t += nt) st[t] = -1;
}

template <int VEC, int XCH, int LD, bool XH = false, bool TW = false>
__global__ __launch_bounds__(kAlNT + LD) void align_kernel(const AlignArgs a) {
  constexpr int NTOT = kAlNT + LD;
  constexpr int NW = NTOT / 64;
  constexpr size_t kXe = XH ? 2 : 4;
  const bool bf16 = a.x_half == kXBf16;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const int L = __builtin_amdgcn_readfirstlane(seq_len(a.lengths, b, a.T));
  const int H = a.H, K = a.K, D = a.D, T = a.T, Dp = (D + 3) & ~3;
  const size_t g = (size_t)b * a.graph_stride;

  // ---- LDS: [score vectors (fp64, ping-pong), nnet-output rows (ping-pong) | reused by the backtrace] [reductions] [arcs]
  char* p = smem_raw;
  const int Hq = (H + 1) & ~1;
  char* walk = p;
  double* va = reinterpret_cast<double*>(p);
  double* vb = va + Hq;
  float* xr0 = reinterpret_cast<float*>(vb + Hq);
  float* xr1 = xr0 + Dp;
  p += a.walk_bytes;
  double* redd = reinterpret_cast<double*>(p); p += 8 * 16;
  int* redi = reinterpret_cast<int*>(p); p += 4 * 16;    // a wave's argmax, -1 where it met a NaN
  AArc* arc = reinterpret_cast<AArc*>(p); p += 8 * (size_t)K;     // by destination: (src, pdf, lp)
  {
    const int32_t* tr = a.bwd_trans + g * K * 3;
    const float* pr = a.bwd_probs + g * K;
    for (int k = tid; k < K; k += NTOT) arc[k] = AArc{(uint32_t)tr[3 * k] | ((uint32_t)tr[3 * k + 2] << 16), pr[k]};
  }
  const float* xseq = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.x) + (size_t)b * T * D * kXe);
  const XBuf xbuf = make_xbuf(xseq, (size_t)T * D * kXe);
  auto xload = [&](auto& xr, int t, int ti) {
    if constexpr (XH) xr.load_h(reinterpret_cast<const char*>(xseq) + (size_t)t * D * 2, D, ti);
    else xr.load(xseq + (size_t)t * D, D, ti);
  };
  auto xload_row = [&](auto& xr, int t, int ti) {
    if constexpr (XH) xr.load_row_h(xbuf, t, D, ti);
    else xr.load_row(xbuf, t, D, ti);
  };
  // a row, clamped, into LDS; a NaN stays a NaN (it makes the arc terms that read it NaN: the per-thread flag below)
  auto stage = [&](auto& xr, float* lds, const float* row, int t) {
    if constexpr (XH) xr.convert_h(bf16);
    xr.store(lds, row, D, t, kXClamp);
  };
  uint16_t* bps = a.bp16 + (size_t)b * T * a.Hb;
  const int2* idx = reinterpret_cast<const int2*>(a.bwd_idx + g * H * 2);
  const int32_t* win = TW ? a.windows + (size_t)b * H * 2 : nullptr;         // {lo, hi} per state: one row per sequence
  auto adm_at = [&](int h, int t) { return win[2 * h] <= t && t <= win[2 * h + 1]; };

  const int h0 = tid;
  const bool own = h0 < H && tid < kAlNT;
  int2 be = make_int2(0, 0);
  if (own) be = idx[h0];
  int wlo = 0, whi = 0;
  if constexpr (TW) if (own) { wlo = win[2 * h0]; whi = win[2 * h0 + 1]; }
  XRow<LD ? LD : kAlNT, VEC, XCH> xq;
  const int xt = LD ? tid - kAlNT : tid;
  {
    const float* xrow = XH ? nullptr : xseq;
    if (!LD || tid >= kAlNT) xload(xq, 0, xt);
    if (tid < kAlNT)
      for (int h = tid; h < H; h += kAlNT) {
        double v = (double)a.initial[g * H + h];
        if constexpr (TW) if (!adm_at(h, 0)) v = -INFINITY;
        va[h] = v;
      }
    if (!LD || tid >= kAlNT) stage(xq, xr0, xrow, xt);
  }
  __syncthreads();
  int nanf = 0;
  if (LD > 0 && tid >= kAlNT) {
    if constexpr (LD > 0) {
      // ---- row-staging waves (num_kernels.hip: num_fb_kernel): step s reads xr0 (s odd) / xr1 (s even)
      static_assert(VEC == 4 && XCH > 0, "row-staging waves use the float4 buffer-load form");
      XRow<LD, VEC, XCH> xq2;
      auto row_of_step = [&](int s) { return min(s, L) - 1; };
      xload_row(xq, row_of_step(2), xt);
      for (int s = 1; s <= L; s += 2) {
        xload_row(xq2, row_of_step(s + 2), xt);
        stage(xq, xr1, nullptr, xt);                 // row of step s+1
        __syncthreads();
        if (s + 1 <= L) {
          xload_row(xq, row_of_step(s + 3), xt);
          stage(xq2, xr0, nullptr, xt);              // row of step s+2
          __syncthreads();
        }
      }
    }
  } else {
    AArc w0{0u, 0.f}, w1{0u, 0.f};
    const int n0 = be.y - be.x;
    if (own) {
      if (n0 > 0) w0 = arc[be.x];
      if (n0 > 1) w1 = arc[be.x + 1];
    }
    // s(t+1,h) = max_k s(t,src_k) + (lp_k + x(t,pdf_k)), t = s - 1
    for (int s = 1; s <= L; s++) {
      const double* vin = (s & 1) ? va : vb;
      double* vout = (s & 1) ? vb : va;
      const float* xcur = (s & 1) ? xr0 : xr1;
      float* xnext = (s & 1) ? xr1 : xr0;
      const bool have_next = s < L;
      const int t_next = have_next ? s : 0;
      const float* xrow_next = XH ? nullptr : xseq + (size_t)t_next * D;
      uint16_t* brow = bps + (size_t)(s - 1) * a.Hb;
      if (!LD && have_next) {
        if constexpr (VEC == 4 && XCH > 0) xload_row(xq, t_next, tid);
        else xq.load(xrow_next, D, tid);
      }
      if (own) {
        double best = -INFINITY;
        int bi = 0;
        const bool adm = !TW || (wlo <= s && s <= whi);          // (a masked state: -inf, backpointer 0, no arc term counts)
        if (adm && n0 > 0) {
          best = vin[w0.pk & 0xffffu] + ((double)w0.lp + (double)xcur[w0.pk >> 16]);
          nanf |= best != best;
        }
        if (adm && n0 > 1) {
          const double e = vin[w1.pk & 0xffffu] + ((double)w1.lp + (double)xcur[w1.pk >> 16]);
          nanf |= e != e;
          if (e > best) { best = e; bi = 1; }
        }
        for (int k = be.x + 2; k < (adm ? be.y : 0); k++) {
          const AArc w = arc[k];
          const double e = vin[w.pk & 0xffffu] + ((double)w.lp + (double)xcur[w.pk >> 16]);
          nanf |= e != e;
          if (e > best) { best = e; bi = k - be.x; }
        }
        vout[h0] = best;
        brow[h0] = (uint16_t)bi;
      }
      for (int h = h0 + kAlNT; h < H; h += kAlNT) {             // graphs with more than 512 states
        int2 e2 = idx[h];
        if constexpr (TW) if (!adm_at(h, s)) e2.y = e2.x;
        double best = -INFINITY;
        int bi = 0;
        for (int k = e2.x; k < e2.y; k++) {
          const AArc w = arc[k];
          const double e = vin[w.pk & 0xffffu] + ((double)w.lp + (double)xcur[w.pk >> 16]);
          nanf |= e != e;
          if (k == e2.x || e > best) { best = e; bi = k - e2.x; }
        }
        vout[h] = best;
        brow[h] = (uint16_t)bi;
      }
      if (!LD && have_next) stage(xq, xnext, xrow_next, tid);
      __syncthreads();
    }
  }

  // ---- score = max_h s(L,h) + final(h), the lowest h on ties; NaN if any arc term was NaN
  const double* vL = (L & 1) ? vb : va;
  double mx = -INFINITY;
  int mi = 0x7fffffff;
  if (tid < kAlNT)
    for (int h = tid; h < H; h += kAlNT) {
      if constexpr (TW) if (!adm_at(h, L)) continue;
      const double e = vL[h] + (double)a.final_[g * H + h];
      nanf |= e != e;
      if (e > mx) { mx = e; mi = h; }
    }
  wave_argmax(mx, mi);
  const int wnan = __builtin_amdgcn_ballot_w64(nanf != 0) != 0;
  if (lane == 0) { redd[wave] = mx; redi[wave] = wnan ? -1 : mi; }
  __threadfence();                                     // (the backpointer rows reach L2 before anyone reads them back)
  __syncthreads();
  double best = redd[0];
  int hstar = redi[0], anynan = redi[0] < 0;
#pragma unroll
  for (int w = 1; w < NW; w++) { argmax_merge(best, hstar, redd[w], redi[w]); anynan |= redi[w] < 0; }
  const double score = anynan ? canonical_nan() : best;
  const bool ok = !anynan && best > -INFINITY && best < INFINITY;
  if (tid == 0) {
    a.score[b] = score;
    if (!ok || seq_len_bad(a.lengths, b, T)) atomicAdd(a.bad, 1);
  }
  pad_rows(a, b, L, ok, tid, NTOT);
  if (!ok) return;                                     // (uniform over the workgroup)
  int64_t* pd = a.pdfs + (size_t)b * T;
  int32_t* st = a.states + (size_t)b * (T + 1);
  if (tid == 0) st[L] = hstar;

  // ---- backtrace over blocks of F frames from the end: iteration j, one barrier each:
  //   waves 1.. : backpointer rows of block j -> the winning arc's pk (src | pdf << 16) into tab[j & 1];
  //               the path of block j - 2 (path[j & 1]) out to states / pdfs, coalesced
  //   lane 0    : walks block j - 1 inside tab[(j - 1) & 1], one dependent LDS read per frame, into path[(j - 1) & 1]
  constexpr int nconv = NTOT - 64;
  int F = a.walk_bytes / (8 * H + 8);
  F = min(F, kAlPre * nconv / H);
  F = max(F, 1);
  uint32_t* tab0 = reinterpret_cast<uint32_t*>(walk);
  uint32_t* tab1 = tab0 + (size_t)F * H;
  uint32_t* path0 = tab1 + (size_t)F * H;
  uint32_t* path1 = path0 + F;
  const int nblk = (L + F - 1) / F;
  const uint32_t* bpw = reinterpret_cast<const uint32_t*>(bps);
  int h = hstar;                                       // (lane 0's walk position: the state at the end of the next block)
  for (int j = 0; j <= nblk + 1; j++) {
    if (tid >= 64) {
      const int c = tid - 64;
      if (j < nblk) {
        const int hi = L - j * F, lo = max(hi - F, 0), ne = (hi - lo) * H;
        uint32_t* tab = (j & 1) ? tab1 : tab0;
        uint32_t wv[kAlPre];
        int lov[kAlPre], hv[kAlPre];
#pragma unroll
        for (int i = 0; i < kAlPre; i++) {
          const int e = c + i * nconv;
          if (e < ne) {
            const int r = e / H, hh = e - r * H;
            hv[i] = hh;
            wv[i] = fresh_u32(bpw + (((size_t)(lo + r) * a.Hb + hh) >> 1));
            lov[i] = idx[hh].x;
          }
        }
#pragma unroll
        for (int i = 0; i < kAlPre; i++) {
          const int e = c + i * nconv;
          if (e < ne) {
            const int off = (hv[i] & 1) ? (int)(wv[i] >> 16) : (int)(wv[i] & 0xffffu);     // (Hb even: a row starts a word)
            tab[e] = arc[min(lov[i] + off, K - 1)].pk;      // (states no path enters may point anywhere: kept in range)
          }
        }
      }
      if (j >= 2) {
        const int jj = j - 2, hi = L - jj * F, lo = max(hi - F, 0);
        const uint32_t* path = (jj & 1) ? path1 : path0;
        for (int i = c; i < hi - lo; i += nconv) {
          const uint32_t pk = path[i];
          st[lo + i] = (int32_t)(pk & 0xffffu);
          pd[lo + i] = (int64_t)(pk >> 16);
        }
      }
    } else if (tid == 0 && j >= 1 && j <= nblk) {
      const int jj = j - 1, hi = L - jj * F, lo = max(hi - F, 0);
      const uint32_t* tab = (jj & 1) ? tab1 : tab0;
      uint32_t* path = (jj & 1) ? path1 : path0;
      for (int t = hi - 1; t >= lo; t--) {
        const uint32_t pk = tab[(t - lo) * H + h];
        path[t - lo] = pk;
        h = (int)(pk & 0xffffu);
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------
// graphs beyond the tile kernel: everything in global memory
// ------------------------------------------------------------------------------------
template <bool TW>
__global__ __launch_bounds__(kAlGT) void align_general_kernel(const AlignArgs a) {
  __shared__ double redd[kAlGT / 64];
  __shared__ int redi[kAlGT / 64], redn[kAlGT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int L = seq_len(a.lengths, b, a.T);
  const int H = a.H, K = a.K, D = a.D, T = a.T;
  const size_t g = (size_t)b * a.graph_stride;
  const int32_t* tr = a.bwd_trans + g * K * 3;
  const float* pr = a.bwd_probs + g * K;
  const int2* idx = reinterpret_cast<const int2*>(a.bwd_idx + g * H * 2);
  const float* xseq = a.x + (size_t)b * T * D;
  double* sc = a.gen_sc + (size_t)b * 2 * H;
  int32_t* bps = a.bp32 + (size_t)b * T * H;
  const int32_t* win = TW ? a.windows + (size_t)b * H * 2 : nullptr;
  auto adm_at = [&](int h, int t) { return win[2 * h] <= t && t <= win[2 * h + 1]; };
  for (int h = tid; h < H; h += kAlGT) {
    double v = (double)a.initial[g * H + h];
    if constexpr (TW) if (!adm_at(h, 0)) v = -INFINITY;
    sc[h] = v;
  }
  __threadfence();
  __syncthreads();
  int nanf = 0;
  for (int s = 1; s <= L; s++) {
    const double* vin = sc + (size_t)((s - 1) & 1) * H;
    double* vout = sc + (size_t)(s & 1) * H;
    const float* xrow = xseq + (size_t)(s - 1) * D;
    int32_t* brow = bps + (size_t)(s - 1) * H;
    for (int h = tid; h < H; h += kAlGT) {
      int2 be = idx[h];
      if constexpr (TW) if (!adm_at(h, s)) be.y = be.x;
      double best = -INFINITY;
      int bi = 0;
      for (int k = be.x; k < be.y; k++) {
        const double e = fresh_f64(vin + tr[3 * k]) + ((double)pr[k] + (double)aclamp(xrow[tr[3 * k + 2]]));
        nanf |= e != e;
        if (k == be.x || e > best) { best = e; bi = k - be.x; }
      }
      vout[h] = best;
      brow[h] = bi;
    }
    __threadfence();
    __syncthreads();
  }
  const double* vL = sc + (size_t)(L & 1) * H;
  double mx = -INFINITY;
  int mi = 0x7fffffff;
  for (int h = tid; h < H; h += kAlGT) {
    if constexpr (TW) if (!adm_at(h, L)) continue;
    const double e = fresh_f64(vL + h) + (double)a.final_[g * H + h];
    nanf |= e != e;
    if (e > mx) { mx = e; mi = h; }
  }
  wave_argmax(mx, mi);
  const int wnan = __builtin_amdgcn_ballot_w64(nanf != 0) != 0;
  if (lane == 0) { redd[wave] = mx; redi[wave] = mi; redn[wave] = wnan; }
  __syncthreads();
  double best = redd[0];
  int hstar = redi[0], anynan = redn[0];
  for (int w = 1; w < kAlGT / 64; w++) { argmax_merge(best, hstar, redd[w], redi[w]); anynan |= redn[w]; }
  const bool ok = !anynan && best > -INFINITY && best < INFINITY;
  if (tid == 0) {
    a.score[b] = anynan ? canonical_nan() : best;
    if (!ok || seq_len_bad(a.lengths, b, T)) atomicAdd(a.bad, 1);
  }
  pad_rows(a, b, L, ok, tid, kAlGT);
  if (!ok || tid != 0) return;
  int64_t* pd = a.pdfs + (size_t)b * T;
  int32_t* st = a.states + (size_t)b * (T + 1);
  st[L] = hstar;
  int h = hstar;
  for (int t = L - 1; t >= 0; t--) {
    const int k = idx[h].x + fresh_i32(bps + (size_t)t * H + h);
    pd[t] = (int64_t)tr[3 * k + 2];
    h = tr[3 * k];
    st[t] = h;
  }
}

template <int VEC, int XCH, int LD, bool XH, bool TW>
hipError_t launch_align_w(const AlignArgs& a, size_t lds, hipStream_t st) {
  auto k = align_kernel<VEC, XCH, LD, XH, TW>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3(a.B), dim3(kAlNT + LD), lds, st, a);
  return hipGetLastError();
}
template <int VEC, int XCH, int LD, bool XH>
hipError_t launch_align_x(const AlignArgs& a, size_t lds, hipStream_t st) {
  return a.windows ? launch_align_w<VEC, XCH, LD, XH, true>(a, lds, st) : launch_align_w<VEC, XCH, LD, XH, false>(a, lds, st);
}
template <int VEC, int XCH, int LD = 0>
hipError_t launch_align_t(const AlignArgs& a, size_t lds, hipStream_t st) {
  if (a.x_half) {
    if constexpr (VEC == 4 && XCH > 0) return launch_align_x<VEC, XCH, LD, true>(a, lds, st);
    else return hipErrorInvalidValue;
  }
  return launch_align_x<VEC, XCH, LD, false>(a, lds, st);
}

size_t align_fixed_lds_bytes(int K) { return 8 * 16 + 4 * 16 + 8 * (size_t)K + 64; }     // (with the forward's region: num_fb_lds_bytes)

// the region the forward's score vectors and rows live in, enlarged (up to kAlWalkCap, within the 160 KiB) for the backtrace
int align_walk_bytes(int H, int K, int D) {
  const size_t Dp = (D + 3) & ~3, Hq = (H + 1) & ~1;
  const size_t fwd = 16 * Hq + 8 * Dp;
  const size_t room = 160 * 1024 > align_fixed_lds_bytes(K) ? 160 * 1024 - align_fixed_lds_bytes(K) : 0;
  size_t w = kAlWalkCap < room ? kAlWalkCap : room;
  if (w < fwd) w = fwd;
  // (rounded DOWN: `room` is 8 mod 16 for an odd K, and rounding it up took 8 bytes more than the CU has - a graph of 4000
  // states and 8399 arcs was refused; fwd is a multiple of 16, so the forward's buffers still fit)
  return (int)(w & ~(size_t)15);
}
size_t align_lds_bytes(int H, int K, int D) { return (size_t)align_walk_bytes(H, K, D) + align_fixed_lds_bytes(K); }

hipError_t launch_align(const AlignArgs& a, hipStream_t st, const char** why) {
  if (a.general) {
    if (a.windows) hipLaunchKernelGGL(align_general_kernel<true>, dim3(a.B), dim3(kAlGT), 0, st, a);
    else hipLaunchKernelGGL(align_general_kernel<false>, dim3(a.B), dim3(kAlGT), 0, st, a);
    return hipGetLastError();
  }
  const size_t lds = align_lds_bytes(a.H, a.K, a.D);
  if (lds > 160 * 1024) {
    *why = "numerator graph + nnet-output rows do not fit the 160 KiB LDS of one CU";
    return hipErrorInvalidValue;
  }
  if (a.x_half && (a.D % 4 != 0 || a.D > 4 * 8 * kAlNT)) {
    *why = "2-byte network outputs need rows of a multiple of four pdfs within the register-staged forms";
    return hipErrorInvalidValue;
  }
  if ((size_t)a.T * a.D * 4 >= (size_t)1 << 31) {
    *why = "one sequence's nnet-output slab reaches 2 GiB";
    return hipErrorInvalidValue;
  }
  const int D = a.D;
  if (D % 4 == 0) {
    if (D <= 4 * 4 * kAlLd) return launch_align_t<4, 4, kAlLd>(a, lds, st);
    if (D <= 4 * 8 * kAlLd) return launch_align_t<4, 8, kAlLd>(a, lds, st);
    if (D <= 4 * 8 * kAlNT) return launch_align_t<4, 8>(a, lds, st);
  } else if (D <= 8 * kAlNT) {
    return launch_align_t<1, 8>(a, lds, st);
  }
  return launch_align_t<1, 0>(a, lds, st);
}

// ---- the entry points (include/pychain_hip.h: pychain_hip_align*) ------------------------------------------------------------

struct AlignCarve { size_t bp, sc, total; };
AlignCarve align_carve(int B, int T, int H, int K, int D) {
  AlignCarve c;
  c.bp = 0;
  if (num_needs_general(H, K, D)) {                  // int32 backpointers + the two score vectors per sequence
    c.sc = align256(4 * (size_t)B * T * H);
    c.total = c.sc + align256(16 * (size_t)B * H) + 256;
  } else {                                          // uint16 backpointers, rows of H rounded up to even
    c.sc = align256(2 * (size_t)B * T * (size_t)((H + 1) & ~1));
    c.total = c.sc + 256;
  }
  return c;
}
bool align_half_native(int H, int K, int D) { return !num_needs_general(H, K, D) && D % 4 == 0 && D <= 4 * 8 * 512; }
}  // namespace
}  // namespace pychain_hip

using namespace pychain_hip;

extern "C" size_t pychain_hip_align_workspace_bytes(int B, int T, int H, int K, int D) {
  if (B <= 0 || T <= 0 || H <= 0 || K <= 0 || D <= 0) return 0;
  return align_carve(B, T, H, K, D).total;
}
extern "C" int pychain_hip_align_half_native(int H, int K, int D) {
  if (H <= 0 || K <= 0 || D <= 0) return 0;
  return align_half_native(H, K, D) ? 1 : 0;
}

extern "C" int pychain_hip_align_tw(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int D, int H, int K, double* score_per_seq, int32_t* states, int64_t* pdfs, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream, const int32_t* time_windows) {
  const char* who = "align";
  (void)ft; (void)fi; (void)fp;                      // (the recursion gathers over the arcs entering each state only)
  if (int rc = bad_dtype(who, nnet_output_dtype)) return rc;
  if (!bt || !bi || !bp || !initial || !final_ || !nnet_output || !seq_lengths || !score_per_seq || !states || !pdfs ||
      !bad_count || !workspace)
    return null_pointer(who);
  if (int rc = bad_sizes(who, B, T, H, K, D)) return rc;
  if (int rc = bad_stride(who, graph_batch_stride)) return rc;
  if (((uintptr_t)nnet_output | (uintptr_t)bi) & 15)
    return fail(PYCHAIN_HIP_EINVAL, "%s: nnet_output and index tensors must be 16-byte aligned", who);
  const AlignCarve c = align_carve(B, T, H, K, D);
  if (workspace_bytes < c.total) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace too small", who);
  if (nnet_output_dtype != PYCHAIN_HIP_F32 && !align_half_native(H, K, D))
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: this shape does not take 2-byte network outputs (pychain_hip_align_half_native)", who);
  AlignArgs a;
  memset(&a, 0, sizeof(a));
  a.bwd_trans = bt; a.bwd_idx = bi; a.bwd_probs = bp; a.initial = initial; a.final_ = final_;
  a.x = (const float*)nnet_output; a.x_half = nnet_output_dtype; a.lengths = seq_lengths;
  a.score = score_per_seq; a.states = states; a.pdfs = pdfs; a.bad = bad_count;
  a.graph_stride = graph_batch_stride; a.B = B; a.T = T; a.D = D; a.H = H; a.K = K;
  a.Hb = (H + 1) & ~1;
  a.general = num_needs_general(H, K, D) ? 1 : 0;
  a.windows = time_windows;                          // (nullptr: the kernels without the mask, exactly the call before ABI 26)
  char* ws = ws_base(workspace);
  if (a.general) { a.bp32 = (int32_t*)(ws + c.bp); a.gen_sc = (double*)(ws + c.sc); }
  else { a.bp16 = (uint16_t*)(ws + c.bp); a.walk_bytes = align_walk_bytes(H, K, D); }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(bad_count, 0, sizeof(int32_t), st) != hipSuccess)
    return fail(PYCHAIN_HIP_ELAUNCH, "%s: hipMemsetAsync failed", who);
  const char* why = nullptr;
  const hipError_t e = launch_align(a, st, &why);
  return e == hipSuccess ? PYCHAIN_HIP_OK : launch_failed(who, e, why);
}

extern "C" int pychain_hip_align(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int D, int H, int K, double* score_per_seq, int32_t* states, int64_t* pdfs, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream) {
  return pychain_hip_align_tw(ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, nnet_output, nnet_output_dtype, seq_lengths,
                              B, T, D, H, K, score_per_seq, states, pdfs, bad_count, workspace, workspace_bytes, stream, nullptr);
}
