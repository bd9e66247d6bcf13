// cpu.cpp - the HOST twins of the two forward-backward entry points (include/pychain_hip.h: pychain_hip_cpu_*; SURVEY.md
// §8(b) lists them in the boundary).  The reference runs on whatever device its input tensor lives on
// (chain-computation.cc:40,102,183,318; chain-log-domain-computation.cc:123-159,231-271) and code written against it
// unit-tests its criterion on CPU tensors; `pychain_amd` therefore serves CPU tensors from HERE and device tensors from the
// HIP kernels - never one for the other: a device tensor that cannot reach the kernels raises, it does not come here
// (pychain_amd/native.py), and the test suite's CPU checker is no part of it.
//
// Own design, not the reference's loop nest: the sequences of a minibatch are independent (chain-computation.h:33-35), so they
// are dealt to host threads; clamp(-30, 30) and exp (pychain/loss.py:30,43) are applied to a frame's row once, into a scratch
// row, instead of to the whole [B,T,D] tensor in two passes; the per-frame totals, the log-probability and every
// normaliser are accumulated in fp64 (the state vectors and the gradient are fp32, as the reference's); the numerator keeps
// fp64 log-probabilities and an exact max-subtracted log-sum-exp like the device path (num_kernels.hip) - the reference's
// fp32 LogAdd chain with its cut-off is the device's option num_compat, not rebuilt here.  Equations: chain-computation.h:109-156.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "../../include/pychain_hip.h"
#include "call_args.h"
#include "common.h"

namespace pychain_hip {
namespace {
std::atomic<long> g_cpu_calls{0};

struct Csr {                       // one graph in the reference layout: arcs {src, dst, pdf} in runs per state
  const int32_t* trans;
  const int32_t* idx;
  const float* prob;
};
inline Csr fwd_of(const NumGraphs& g) { return Csr{g.ft, g.fi, g.fp}; }     // arcs leaving each state
inline Csr bwd_of(const NumGraphs& g) { return Csr{g.bt, g.bi, g.bp}; }     // arcs entering each state
inline float clamp30(float v) { return v != v ? v : (v < -30.f ? -30.f : (v > 30.f ? 30.f : v)); }
inline int clamped_length(int64_t l, int T) { return l < 1 ? 1 : (l > T ? T : (int)l); }     // (the row passes: as on the device)

template <class F>
void for_each_sequence(int B, int num_threads, F&& body) {
  int nt = num_threads > 0 ? num_threads : (int)std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > B) nt = B;
  if (nt == 1) { for (int b = 0; b < B; b++) body(b); return; }
  std::atomic<int> next{0};
  std::vector<std::thread> pool;
  for (int i = 0; i < nt; i++)
    pool.emplace_back([&]() { for (int b = next.fetch_add(1); b < B; b = next.fetch_add(1)) body(b); });
  for (auto& th : pool) th.join();
}

// ---- denominator: probability domain, leaky-HMM, per-frame renormalisation (chain-computation.h:124-153) ------------------
// alpha'(t) = alpha(t) + tot(t) coef leaky; alpha(t+1,j) = sum_{k into j} alpha'(t,src) p x(t,pdf) / tot(t);
// beta'(t,i) = sum_{k out of i} p x(t,pdf) beta(t+1,dst) / tot(t); beta(t) = beta'(t) + coef sum_i leaky_i beta'(t,i);
// gamma(t,pdf) += alpha'(t,src) p x(t,pdf) beta(t+1,dst) / tot(t).
bool den_one(const Csr& fwd, const Csr& bwd, const float* leaky, const float* init, const float* fin, const float* x, int input_is_exp,
             int L, int T, int D, int H, float coef, float gscale, float* objf, float* grad) {
  std::vector<float> alpha((size_t)(L + 1) * H), beta(2 * (size_t)H), row((size_t)D);
  std::vector<double> tot((size_t)L + 1);
  bool ok = true;
  auto stage = [&](int t) {
    const float* xr = x + (size_t)t * D;
    if (input_is_exp) { for (int n = 0; n < D; n++) row[n] = xr[n]; }
    else { for (int n = 0; n < D; n++) row[n] = std::exp(clamp30(xr[n])); }
  };
  auto dash = [&](int t) {                     // total, then the leaky term: the stored row is alpha'
    float* a = alpha.data() + (size_t)t * H;
    double s = 0.0;
    for (int h = 0; h < H; h++) s += (double)a[h];
    tot[t] = s;
    const float add = (float)(s * (double)coef);
    for (int h = 0; h < H; h++) a[h] += add * leaky[h];
    if (!(s > 0.0) || !std::isfinite(s)) ok = false;
  };
  for (int h = 0; h < H; h++) alpha[h] = init[h];
  dash(0);
  for (int t = 1; t <= L; t++) {
    stage(t - 1);
    const float* pa = alpha.data() + (size_t)(t - 1) * H;
    float* a = alpha.data() + (size_t)t * H;
    const float inv = (float)(1.0 / tot[t - 1]);
    for (int h = 0; h < H; h++) {
      float acc = 0.f;
      for (int k = bwd.idx[2 * h]; k < bwd.idx[2 * h + 1]; k++)
        acc += pa[bwd.trans[3 * k]] * bwd.prob[k] * row[bwd.trans[3 * k + 2]];
      a[h] = acc * inv;
    }
    dash(t);
  }
  // log-probability: log sum_i alpha'(L,i) final(i) + sum_{t<L} log tot(t)   (chain-computation.cc:209-230)
  const float* aL = alpha.data() + (size_t)L * H;
  double last = 0.0;
  for (int h = 0; h < H; h++) last += (double)aL[h] * (double)fin[h];
  double lp = std::log(last);
  for (int t = 0; t < L; t++) lp += std::log(tot[t]);
  *objf = (float)lp;
  if (!std::isfinite(lp)) ok = false;
  // beta(L) = final / last, + its leaky sum (:232-245, :313-330)
  auto leak = [&](float* b) {
    double s = 0.0;
    for (int h = 0; h < H; h++) s += (double)b[h] * (double)leaky[h];
    const float add = (float)(s * (double)coef);
    for (int h = 0; h < H; h++) b[h] += add;
  };
  float* bn = beta.data() + (size_t)(L & 1) * H;
  for (int h = 0; h < H; h++) bn[h] = (float)((double)fin[h] / last);
  leak(bn);
  for (size_t i = 0; i < (size_t)T * D; i++) grad[i] = 0.f;
  for (int t = L - 1; t >= 0; t--) {
    stage(t);
    const float* a = alpha.data() + (size_t)t * H;
    const float* nb = beta.data() + (size_t)((t + 1) & 1) * H;
    float* b = beta.data() + (size_t)(t & 1) * H;
    float* g = grad + (size_t)t * D;
    const float inv = (float)(1.0 / tot[t]);
    for (int h = 0; h < H; h++) {
      const float occ = a[h] * inv;
      float acc = 0.f;
      for (int k = fwd.idx[2 * h]; k < fwd.idx[2 * h + 1]; k++) {
        const int pdf = fwd.trans[3 * k + 2];
        const float v = fwd.prob[k] * nb[fwd.trans[3 * k + 1]] * row[pdf];
        acc += v;
        g[pdf] += v * occ;
      }
      b[h] = acc * inv;
    }
    if (t == 0) {                              // the reference's check: a frame's occupancies sum to one within 5 % (:345-391)
      double s = 0.0;
      for (int n = 0; n < D; n++) s += (double)g[n];
      if (!(std::fabs(s - 1.0) <= 0.05)) ok = false;
    }
    leak(b);
    if (gscale != 1.f) for (int n = 0; n < D; n++) g[n] *= gscale;
  }
  return ok;
}

// ---- numerator: log domain, no leaky-HMM (chain-log-domain-computation.cc), fp64 log-probabilities ------------------------
struct Lse64 {
  double m = -std::numeric_limits<double>::infinity(), s = 0.0;
  void push(double e) {
    if (e != e) { m = e; return; }
    if (e == -std::numeric_limits<double>::infinity()) return;
    if (e > m) { s = (m == -std::numeric_limits<double>::infinity()) ? 1.0 : s * std::exp(m - e) + 1.0; m = e; }
    else s += std::exp(e - m);
  }
  double value() const { return (m != m || m == -std::numeric_limits<double>::infinity()) ? m : m + std::log(s); }
};
// win: the sequence's alignment time windows, {lo, hi} per state, or nullptr (include/pychain_hip.h: pychain_hip_*_tw): a state
// outside its window gets -inf, selected after its log-sum as on the device, and its arcs carry no occupancy
// counts (pychain_hip_cpu_num_arc_counts): fp64 [fwd arcs] or nullptr - every forward arc's occupancy summed over the frames, left
// as it is (zeros) for a sequence without a finite log-probability; logp_out: the fp64 log-probability; grad may then be nullptr:
// the occupancy checks do not run and only the recursion's verdict is returned
bool num_one(const Csr& fwd, const Csr& bwd, const float* init, const float* fin, const float* x, int L, int T, int D, int H,
             int grad_mode_flags, float gscale, float* objf, float* grad, const int32_t* win, double* counts = nullptr,
             double* logp_out = nullptr) {
  // (PYCHAIN_HIP_CPU_NO_CLAMP: the network output as it is - the contract of pychain_C.forward_backward_log_domain, whose C++
  // does not clamp (chain-log-domain-computation.cc:137-145); ChainFunction's clamp(-30, 30), pychain/loss.py:30, otherwise)
  const bool clamp = (grad_mode_flags & PYCHAIN_HIP_CPU_NO_CLAMP) == 0;
  const int grad_mode = grad_mode_flags & 0xff;
  auto xv = [clamp](float v) { return clamp ? clamp30(v) : v; };
  const double ninf = -std::numeric_limits<double>::infinity();
  auto adm = [win](int h, int t) { return !win || (win[2 * h] <= t && t <= win[2 * h + 1]); };
  std::vector<double> alpha((size_t)(L + 1) * H), beta(2 * (size_t)H), occ((size_t)D);
  bool ok = true;
  for (int h = 0; h < H; h++) alpha[h] = adm(h, 0) ? (double)init[h] : ninf;
  for (int t = 1; t <= L; t++) {
    const float* xr = x + (size_t)(t - 1) * D;
    const double* pa = alpha.data() + (size_t)(t - 1) * H;
    double* a = alpha.data() + (size_t)t * H;
    for (int h = 0; h < H; h++) {
      Lse64 acc;
      for (int k = bwd.idx[2 * h]; k < bwd.idx[2 * h + 1]; k++)
        acc.push(pa[bwd.trans[3 * k]] + ((double)bwd.prob[k] + (double)xv(xr[bwd.trans[3 * k + 2]])));
      a[h] = adm(h, t) ? acc.value() : ninf;
    }
  }
  Lse64 tl;
  for (int h = 0; h < H; h++) tl.push(alpha[(size_t)L * H + h] + (double)fin[h]);
  const double logp = tl.value();
  if (objf) *objf = (float)logp;
  if (logp_out) *logp_out = logp;
  if (!std::isfinite(logp)) ok = false;
  if (!grad && (!counts || !ok)) return ok;
  if (!ok) counts = nullptr;
  const float fill = grad_mode == PYCHAIN_HIP_GRAD_LOG ? -std::numeric_limits<float>::infinity() : 0.f;
  if (grad && grad_mode != PYCHAIN_HIP_GRAD_ACCUM) for (size_t i = 0; i < (size_t)T * D; i++) grad[i] = fill;
  double* bn = beta.data() + (size_t)(L & 1) * H;
  for (int h = 0; h < H; h++) bn[h] = adm(h, L) ? (double)fin[h] : ninf;
  std::vector<int> touched;
  for (int t = L - 1; t >= 0; t--) {
    const float* xr = x + (size_t)t * D;
    const double* a = alpha.data() + (size_t)t * H;
    const double* nb = beta.data() + (size_t)((t + 1) & 1) * H;
    double* b = beta.data() + (size_t)(t & 1) * H;
    float* g = grad ? grad + (size_t)t * D : nullptr;
    touched.clear();
    double fsum = 0.0;
    for (int h = 0; h < H; h++) {
      if (!adm(h, t)) { b[h] = ninf; continue; }
      Lse64 acc;
      for (int k = fwd.idx[2 * h]; k < fwd.idx[2 * h + 1]; k++) {
        const int pdf = fwd.trans[3 * k + 2];
        const double term = (double)fwd.prob[k] + nb[fwd.trans[3 * k + 1]] + (double)xv(xr[pdf]);
        acc.push(term);
        const double o = std::exp(a[h] + term - logp);          // occupancy of the arc (0 where a state cannot be reached)
        if (counts && o == o) counts[k] += o;
        if (!grad) continue;
        if (o > 0.0) { if (occ[pdf] == 0.0) touched.push_back(pdf); occ[pdf] += o; fsum += o; }
        else if (o != o) ok = false;
      }
      b[h] = acc.value();
    }
    if (!grad) continue;
    if (t == 0 && !(std::fabs(fsum - 1.0) <= 0.05)) ok = false;    // chain-log-domain-computation.cc:283-304
    for (int pdf : touched) {
      const double o = occ[pdf];
      occ[pdf] = 0.0;
      if (grad_mode == PYCHAIN_HIP_GRAD_LOG) g[pdf] = (float)std::log(o);
      else if (grad_mode == PYCHAIN_HIP_GRAD_LINEAR) g[pdf] = gscale * (float)o;
      else g[pdf] += gscale * (float)o;
    }
  }
  return ok;
}

// ---- Viterbi alignment over a numerator graph (include/pychain_hip.h: pychain_hip_cpu_align; the device's align.hip) ----------
// fp64 adds and compares only, in the association and with the tie rules the device kernels use, so both give the same bits.
// win: the sequence's time windows, {lo, hi} per state, or nullptr (pychain_hip_cpu_align_tw): a state outside its window gets
// -inf, selected after its max, and its arc terms (its final term at L) do not count towards the NaN flag - as on the device
bool align_one(const Csr& bwd, const float* init, const float* fin, const float* x, int L, int T, int D, int H, double* score,
               int32_t* states, int64_t* pdfs, const int32_t* win) {
  const double ninf = -std::numeric_limits<double>::infinity();
  auto adm = [win](int h, int t) { return !win || (win[2 * h] <= t && t <= win[2 * h + 1]); };
  std::vector<double> sa((size_t)H), sb((size_t)H);
  std::vector<int32_t> bp((size_t)L * H);           // winning arc (absolute index) of every (frame, state)
  bool nan = false;
  for (int h = 0; h < H; h++) sa[h] = adm(h, 0) ? (double)init[h] : ninf;
  for (int t = 0; t < L; t++) {
    const float* xr = x + (size_t)t * D;
    const double* vin = (t & 1) ? sb.data() : sa.data();
    double* vout = (t & 1) ? sa.data() : sb.data();
    int32_t* brow = bp.data() + (size_t)t * H;
    for (int h = 0; h < H; h++) {
      const int lo = bwd.idx[2 * h], hi = bwd.idx[2 * h + 1];
      double best = ninf;
      int bk = lo;
      if (!adm(h, t + 1)) { vout[h] = ninf; brow[h] = lo; continue; }
      for (int k = lo; k < hi; k++) {
        const double e = vin[bwd.trans[3 * k]] + ((double)bwd.prob[k] + (double)clamp30(xr[bwd.trans[3 * k + 2]]));
        nan = nan || e != e;
        if (k == lo || e > best) { best = e; bk = k; }
      }
      vout[h] = best;
      brow[h] = bk;
    }
  }
  const double* vL = (L & 1) ? sb.data() : sa.data();
  double best = ninf;
  int hstar = 0;
  for (int h = 0; h < H; h++) {
    if (!adm(h, L)) continue;
    const double e = vL[h] + (double)fin[h];
    nan = nan || e != e;
    if (e > best) { best = e; hstar = h; }
  }
  const bool ok = !nan && std::isfinite(best);
  *score = nan ? std::numeric_limits<double>::quiet_NaN() : best;
  for (int t = ok ? L : 0; t < T; t++) pdfs[t] = -1;
  for (int t = ok ? L + 1 : 0; t <= T; t++) states[t] = -1;
  if (!ok) return false;
  int h = hstar;
  states[L] = h;
  for (int t = L - 1; t >= 0; t--) {
    const int k = bp[(size_t)t * H + h];
    pdfs[t] = bwd.trans[3 * k + 2];
    h = bwd.trans[3 * k];
    states[t] = h;
  }
  return true;
}

// (`out0`, `out1`: the first two outputs of the call; the graph stride is checked behind whatever the call checks next)
int check_common(const char* who, const NumGraphs& g, const Rows& rows, const void* out0, const void* out1, const void* bad) {
  if (g.any_null() || !rows.x || !rows.lengths || !out0 || !out1 || !bad) return null_pointer(who);
  if (int rc = bad_sizes(who, rows, g)) return rc;
  for (int b = 0; b < rows.B; b++)
    if (rows.lengths[b] < 1 || rows.lengths[b] > rows.T) return fail(PYCHAIN_HIP_EINVAL, "%s: sequence lengths must be in [1, %d]", who, rows.T);
  return PYCHAIN_HIP_OK;
}
// ---- the numerator posteriors as cross-entropy targets of z (include/pychain_hip.h: pychain_hip_xent; the device's xent.hip):
// one sequence, fp64 throughout.  gamma [T, D]: the occupancies of the sequence (zero rows where it has no admissible path).
double xent_one(const float* gamma, bool feasible, const float* z, int L, int T, int D, float scale, float* zgrad) {
  double objf = 0.0;
  if (zgrad) std::fill(zgrad, zgrad + (size_t)T * D, 0.f);
  if (!feasible) return 0.0;
  for (int t = 0; t < L; t++) {
    const float* zr = z + (size_t)t * D;
    const float* gr = gamma + (size_t)t * D;
    double m = -std::numeric_limits<double>::infinity(), se = 0.0, s = 0.0, dot = 0.0;
    for (int d = 0; d < D; d++) if ((double)zr[d] > m) m = (double)zr[d];          // (a NaN is passed by here and met by the sum)
    for (int d = 0; d < D; d++) {
      se += std::exp((double)zr[d] - m);
      if (gr[d] != 0.f) { s += (double)gr[d]; dot += (double)gr[d] * (double)zr[d]; }
    }
    const double lse = m + std::log(se);
    objf += dot - s * lse;
    if (zgrad) {
      float* o = zgrad + (size_t)t * D;
      for (int d = 0; d < D; d++) o[d] = (float)((double)scale * ((double)gr[d] - s * std::exp((double)zr[d] - lse)));
    }
  }
  return objf;
}
}  // namespace
}  // namespace pychain_hip

using namespace pychain_hip;

extern "C" long pychain_hip_cpu_calls(void) { return g_cpu_calls.load(); }

extern "C" int pychain_hip_cpu_den_forward_backward(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, int graph_batch_stride,
    const float* nnet_output, int input_is_exp, const int64_t* seq_lengths, int B, int T, int D, int H, int K,
    float leaky_hmm_coefficient, float grad_scale, float* objf_per_seq, float* grad, int32_t* bad_count, int num_threads) {
  const char* who = "cpu_den_forward_backward";
  const NumGraphs graphs{ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, H, K};
  int rc = check_common(who, graphs, Rows{nnet_output, PYCHAIN_HIP_F32, seq_lengths, B, T, D}, objf_per_seq, grad, bad_count);
  if (rc != PYCHAIN_HIP_OK) return rc;
  if (!leaky) return fail(PYCHAIN_HIP_EINVAL, "%s: null leaky_probs", who);
  if ((rc = bad_stride(who, graph_batch_stride)) != PYCHAIN_HIP_OK) return rc;
  if (!(leaky_hmm_coefficient > 0.f && leaky_hmm_coefficient < 1.f))
    return fail(PYCHAIN_HIP_EINVAL, "%s: leaky_hmm_coefficient must be in (0,1), got %g", who, (double)leaky_hmm_coefficient);
  g_cpu_calls++;
  std::atomic<int> bad{0};
  for_each_sequence(B, num_threads, [&](int b) {
    const NumGraphs g = graphs.at(b);
    const float* lk = leaky + (g.initial - initial);         // ([G,H], laid out as the initial probabilities are)
    const bool ok = den_one(fwd_of(g), bwd_of(g), lk, g.initial, g.final_, nnet_output + (size_t)b * T * D, input_is_exp,
                            (int)seq_lengths[b], T, D, H, leaky_hmm_coefficient, grad_scale, objf_per_seq + b, grad + (size_t)b * T * D);
    if (!ok) bad++;
  });
  *bad_count = bad.load();
  return PYCHAIN_HIP_OK;
}

extern "C" int pychain_hip_cpu_num_forward_backward_tw(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D, int H, int K, int grad_mode, float grad_scale,
    float* objf_per_seq, float* grad, int32_t* bad_count, int num_threads, const int32_t* time_windows) {
  const char* who = "cpu_num_forward_backward";
  const NumGraphs graphs{ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, H, K};
  int rc = check_common(who, graphs, Rows{nnet_output, PYCHAIN_HIP_F32, seq_lengths, B, T, D}, objf_per_seq, grad, bad_count);
  if (rc != PYCHAIN_HIP_OK) return rc;
  if ((rc = bad_stride(who, graph_batch_stride)) != PYCHAIN_HIP_OK) return rc;
  if ((grad_mode & ~PYCHAIN_HIP_CPU_NO_CLAMP) < PYCHAIN_HIP_GRAD_LOG || (grad_mode & ~PYCHAIN_HIP_CPU_NO_CLAMP) > PYCHAIN_HIP_GRAD_ACCUM)
    return fail(PYCHAIN_HIP_EINVAL, "%s: unknown grad_mode %d", who, grad_mode);
  g_cpu_calls++;
  std::atomic<int> bad{0};
  for_each_sequence(B, num_threads, [&](int b) {
    const NumGraphs g = graphs.at(b);
    const bool ok = num_one(fwd_of(g), bwd_of(g), g.initial, g.final_, nnet_output + (size_t)b * T * D, (int)seq_lengths[b], T, D, H,
                            grad_mode, grad_scale, objf_per_seq + b, grad + (size_t)b * T * D, window_row(time_windows, b, H));
    if (!ok) bad++;
  });
  *bad_count = bad.load();
  return PYCHAIN_HIP_OK;
}

extern "C" int pychain_hip_cpu_num_forward_backward(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D, int H, int K, int grad_mode, float grad_scale,
    float* objf_per_seq, float* grad, int32_t* bad_count, int num_threads) {
  return pychain_hip_cpu_num_forward_backward_tw(ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, nnet_output, seq_lengths,
                                                 B, T, D, H, K, grad_mode, grad_scale, objf_per_seq, grad, bad_count, num_threads, nullptr);
}

// ---- expected arc counts of the numerator (include/pychain_hip.h: pychain_hip_cpu_num_arc_counts; the device's num_arcs.hip):
// the twin of pychain_hip_cpu_num_forward_backward_tw on fl32(lp + w), every arc's posteriors summed in fp64
namespace pychain_hip {
namespace {
inline int used_arcs(const int32_t* idx, int H, int K) {
  int kmax = 0;
  for (int h = 0; h < H; h++) kmax = idx[2 * h + 1] > kmax ? idx[2 * h + 1] : kmax;
  return kmax < K ? kmax : K;
}
// fl32(lp + w) of one sequence in the forward (wf) and in the backward (wb) order; the weights that are not finite (taken as 0)
int weighted_probs(const Csr& fwd, const Csr& bwd, const float* w, int H, int K, float* wf, float* wb) {
  const int Kf = used_arcs(fwd.idx, H, K), Kb = used_arcs(bwd.idx, H, K);
  int bad = 0;
  for (int k = 0; k < K; k++) {
    float v = 0.f;                                                             // (padding arcs are not read)
    if (k < Kf) {
      float wk = w[k];
      if (!std::isfinite(wk)) { bad++; wk = 0.f; }
      v = fwd.prob[k] + wk;
    }
    wf[k] = v;
  }
  for (int k = 0; k < K; k++) {
    float v = 0.f;
    if (k < Kb) {
      const int src = bwd.trans[3 * k], dst = bwd.trans[3 * k + 1], pdf = bwd.trans[3 * k + 2];
      const float p = bwd.prob[k];
      v = p;
      if (src >= 0 && src < H && dst >= 0 && dst < H) {
        int rank = 0;
        for (int j = bwd.idx[2 * dst] > 0 ? bwd.idx[2 * dst] : 0; j < k; j++)
          if (bwd.trans[3 * j] == src && bwd.trans[3 * j + 2] == pdf && bwd.prob[j] == p) rank++;
        const int j1 = fwd.idx[2 * src + 1] < Kf ? fwd.idx[2 * src + 1] : Kf;
        for (int j = fwd.idx[2 * src] > 0 ? fwd.idx[2 * src] : 0; j < j1; j++)
          if (fwd.trans[3 * j + 1] == dst && fwd.trans[3 * j + 2] == pdf && fwd.prob[j] == p && rank-- == 0) {
            if (std::isfinite(w[j])) v = p + w[j];
            break;
          }
      }
    }
    wb[k] = v;
  }
  return bad;
}
}  // namespace
}  // namespace pychain_hip

extern "C" int pychain_hip_cpu_num_arc_counts(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D, int H, int K, int grad_mode, float grad_scale,
    const float* arc_log_weights, double* objf_per_seq, float* grad, double* counts_per_seq, int32_t* bad_count, int num_threads,
    const int32_t* time_windows) {
  const char* who = "cpu_num_arc_counts";
  const NumGraphs graphs{ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, H, K};
  int rc = check_common(who, graphs, Rows{nnet_output, PYCHAIN_HIP_F32, seq_lengths, B, T, D}, objf_per_seq, counts_per_seq, bad_count);
  if (rc != PYCHAIN_HIP_OK) return rc;
  if ((rc = bad_stride(who, graph_batch_stride)) != PYCHAIN_HIP_OK) return rc;
  if (grad_mode != PYCHAIN_HIP_GRAD_LINEAR && grad_mode != PYCHAIN_HIP_GRAD_ACCUM)
    return fail(PYCHAIN_HIP_EINVAL, "%s: grad_mode must be PYCHAIN_HIP_GRAD_LINEAR or PYCHAIN_HIP_GRAD_ACCUM, got %d", who, grad_mode);
  g_cpu_calls++;
  std::atomic<int> bad{0}, bad_w{0};
  for_each_sequence(B, num_threads, [&](int b) {
    const NumGraphs g = graphs.at(b);
    Csr fwd = fwd_of(g), bwd = bwd_of(g);
    std::vector<float> wf, wb;
    if (arc_log_weights) {
      wf.resize(K); wb.resize(K);
      bad_w += weighted_probs(fwd, bwd, arc_log_weights + (size_t)b * K, H, K, wf.data(), wb.data());
      fwd.prob = wf.data(); bwd.prob = wb.data();
    }
    double* counts = counts_per_seq + (size_t)b * K;
    std::fill(counts, counts + K, 0.0);
    const bool ok = num_one(fwd, bwd, g.initial, g.final_, nnet_output + (size_t)b * T * D, (int)seq_lengths[b], T, D, H, grad_mode, grad_scale,
                            nullptr, grad ? grad + (size_t)b * T * D : nullptr, window_row(time_windows, b, H), counts, objf_per_seq + b);
    if (!ok) bad++;
  });
  bad_count[0] = bad.load(); bad_count[1] = bad_w.load();
  return PYCHAIN_HIP_OK;
}

extern "C" int pychain_hip_cpu_align_tw(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D, int H, int K,
    double* score_per_seq, int32_t* states, int64_t* pdfs, int32_t* bad_count, int num_threads, const int32_t* time_windows) {
  const char* who = "cpu_align";
  const NumGraphs graphs{ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, H, K};
  int rc = check_common(who, graphs, Rows{nnet_output, PYCHAIN_HIP_F32, seq_lengths, B, T, D}, score_per_seq, states, bad_count);
  if (rc != PYCHAIN_HIP_OK) return rc;
  if (!pdfs) return null_pointer(who);
  if ((rc = bad_stride(who, graph_batch_stride)) != PYCHAIN_HIP_OK) return rc;
  g_cpu_calls++;
  std::atomic<int> bad{0};
  for_each_sequence(B, num_threads, [&](int b) {
    const NumGraphs g = graphs.at(b);
    const bool ok = align_one(bwd_of(g), g.initial, g.final_, nnet_output + (size_t)b * T * D, (int)seq_lengths[b], T, D, H,
                              score_per_seq + b, states + (size_t)b * (T + 1), pdfs + (size_t)b * T, window_row(time_windows, b, H));
    if (!ok) bad++;
  });
  *bad_count = bad.load();
  return PYCHAIN_HIP_OK;
}

extern "C" int pychain_hip_cpu_align(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D, int H, int K,
    double* score_per_seq, int32_t* states, int64_t* pdfs, int32_t* bad_count, int num_threads) {
  return pychain_hip_cpu_align_tw(ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, nnet_output, seq_lengths, B, T, D, H, K,
                                  score_per_seq, states, pdfs, bad_count, num_threads, nullptr);
}

extern "C" int pychain_hip_cpu_num_forward_backward_xent(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D, int H, int K, int grad_mode, float grad_scale,
    float* objf_per_seq, float* grad, int32_t* bad_count, int num_threads, const int32_t* time_windows,
    const pychain_hip_xent* xent) {
  const char* who = "cpu_num_forward_backward";
  if (xent && (!xent->z || !xent->xent_objf_per_seq)) return fail(PYCHAIN_HIP_EINVAL, "%s: xent: null z or xent_objf_per_seq", who);
  if (xent && xent->z_dtype != PYCHAIN_HIP_F32) return fail(PYCHAIN_HIP_EINVAL, "%s: xent: the host twin takes fp32 z", who);
  const int rc = pychain_hip_cpu_num_forward_backward_tw(ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, nnet_output, seq_lengths,
                                                         B, T, D, H, K, grad_mode, grad_scale, objf_per_seq, grad, bad_count, num_threads,
                                                         time_windows);
  if (rc != PYCHAIN_HIP_OK || !xent) return rc;
  // gamma: the occupancies once more, per sequence, as a linear fp32 row buffer of the thread's own; then the rows of z
  const float sc = xent->grad_scale * (xent->grad_scale_dev ? *xent->grad_scale_dev : 1.f);
  const NumGraphs graphs{ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, H, K};
  for_each_sequence(B, num_threads, [&](int b) {
    const NumGraphs g = graphs.at(b);
    std::vector<float> gamma((size_t)T * D);
    float logp = 0.f;
    num_one(fwd_of(g), bwd_of(g), g.initial, g.final_, nnet_output + (size_t)b * T * D, (int)seq_lengths[b], T, D, H,
            PYCHAIN_HIP_GRAD_LINEAR | (grad_mode & PYCHAIN_HIP_CPU_NO_CLAMP), 1.f, &logp, gamma.data(), window_row(time_windows, b, H));
    xent->xent_objf_per_seq[b] = (float)xent_one(gamma.data(), std::isfinite(logp), (const float*)xent->z + (size_t)b * T * D, (int)seq_lengths[b],
                                                 T, D, sc, xent->xent_grad ? (float*)xent->xent_grad + (size_t)b * T * D : nullptr);
  });
  if (xent->xent_totals) {
    double S = 0.0;
    for (int b = 0; b < B; b++) S += (double)xent->xent_objf_per_seq[b];
    xent->xent_totals[0] = xent->xent_totals[1] = (float)S;
  }
  return PYCHAIN_HIP_OK;
}

// ---- output regularisers (include/pychain_hip.h: pychain_hip_output_reg; the device's outreg.hip): the same fp32 operation
// sequence of the gradient term - nothing contracted - and fp64 sums, frame by frame in ascending order
namespace pychain_hip {
namespace {
inline float outreg_term(float x, float l2, float oor2, float lim, float s) {
#pragma clang fp contract(off)
  const float a = l2 * x;
  const float d = std::fabs(x) - lim;
  const float e = d > 0.f ? d : 0.f;
  const float u = std::fma(oor2, std::copysign(e, x), a);
  return s * u;
}
inline float outreg_add(float g, float term) {
#pragma clang fp contract(off)
  return g + term;
}
}  // namespace
}  // namespace pychain_hip

extern "C" int pychain_hip_cpu_output_reg(
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D,
    float l2, float oor, float limit, int grad_mode, float* grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    float* reg_per_seq, float loss_scale, float* reg_totals, float* totals, int num_threads) {
  const char* who = "cpu_output_reg";
  if (!nnet_output || !seq_lengths || !reg_per_seq) return null_pointer(who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (!(l2 >= 0.f) || !(oor >= 0.f) || !(limit >= 0.f))
    return fail(PYCHAIN_HIP_EINVAL, "%s: l2, oor and limit must not be negative (got %g, %g, %g)", who, (double)l2, (double)oor, (double)limit);
  if (grad_mode != PYCHAIN_HIP_GRAD_ACCUM && grad_mode != PYCHAIN_HIP_GRAD_LINEAR)
    return fail(PYCHAIN_HIP_EINVAL, "%s: grad_mode must be PYCHAIN_HIP_GRAD_ACCUM or PYCHAIN_HIP_GRAD_LINEAR, got %d", who, grad_mode);
  g_cpu_calls++;
  float s = grad_scale_dev ? grad_scale * *grad_scale_dev : grad_scale;
  if (loss_norm_dev) s = s / *loss_norm_dev;
  const float oor2 = 2.f * oor;
  const double limd = (double)limit;
  const bool accum = grad_mode == PYCHAIN_HIP_GRAD_ACCUM;
  std::vector<double> pairs(2 * (size_t)B);
  for_each_sequence(B, num_threads, [&](int b) {
    const int L = clamped_length(seq_lengths[b], T);
    const float* x = nnet_output + (size_t)b * T * D;
    float* g = grad ? grad + (size_t)b * T * D : nullptr;
    double s2 = 0.0, so = 0.0;
    for (int t = 0; t < L; t++) {
      double r2 = 0.0, ro = 0.0;
      for (int n = 0; n < D; n++) {
        const float v = x[(size_t)t * D + n];
        const double xd = (double)v, ad = std::fabs(xd) - limd, ed = !(ad <= 0.0) ? ad : 0.0;
        r2 = std::fma(xd, xd, r2);
        ro = std::fma(ed, ed, ro);
        if (g) {
          const float term = outreg_term(v, l2, oor2, limit, s);
          g[(size_t)t * D + n] = accum ? outreg_add(g[(size_t)t * D + n], term) : term;
        }
      }
      s2 += r2; so += ro;
    }
    if (g && !accum) memset(g + (size_t)L * D, 0, sizeof(float) * (size_t)(T - L) * D);
    pairs[2 * (size_t)b] = s2; pairs[2 * (size_t)b + 1] = so;
    reg_per_seq[2 * b] = (float)s2; reg_per_seq[2 * b + 1] = (float)so;
  });
  if (reg_totals || totals) {
    double s2 = 0.0, so = 0.0;
    for (int b = 0; b < B; b++) { s2 += pairs[2 * (size_t)b]; so += pairs[2 * (size_t)b + 1]; }
    double v = (double)loss_scale * ((l2 != 0.f ? 0.5 * (double)l2 * s2 : 0.0) + (oor != 0.f ? (double)oor * so : 0.0));
    if (loss_norm_dev) v /= (double)*loss_norm_dev;
    if (reg_totals) { reg_totals[0] = (float)v; reg_totals[1] = (float)s2; reg_totals[2] = (float)so; }
    if (totals) { const float full = (float)((double)totals[0] + v); totals[0] = full; totals[4] = full; }
  }
  return PYCHAIN_HIP_OK;
}

// ---- utterance and derivative weights (include/pychain_hip.h: pychain_hip_weight_rows; the device's weights.hip): the same
// single fp32 multiply per element, the same fp64 sums in ascending b
extern "C" int pychain_hip_cpu_weight_rows(
    float* grad, const int64_t* seq_lengths, int B, int T, int D,
    const float* utt_weights, const float* deriv_weights,
    const float* den_objf_per_seq, const float* num_objf_per_seq, const float* xent_objf_per_seq, float xent_coef,
    const float* reg_per_seq, float l2, float oor, float loss_scale, const float* loss_norm_dev,
    float* totals, float* weighted, int num_threads) {
  const char* who = "cpu_weight_rows";
  if (!utt_weights && !deriv_weights) return fail(PYCHAIN_HIP_EINVAL, "%s: neither utt_weights nor deriv_weights", who);
  if (!seq_lengths) return fail(PYCHAIN_HIP_EINVAL, "%s: null seq_lengths", who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  const bool sums = totals || weighted;
  if (!grad && !sums) return fail(PYCHAIN_HIP_EINVAL, "%s: nothing to do (no grad, no totals, no weighted)", who);
  if (sums && (!den_objf_per_seq || !num_objf_per_seq)) return fail(PYCHAIN_HIP_EINVAL, "%s: the sums need den_objf_per_seq and num_objf_per_seq", who);
  g_cpu_calls++;
  auto len = [&](int b) { return clamped_length(seq_lengths[b], T); };
  if (grad) {
    for_each_sequence(B, num_threads, [&](int b) {
      const int L = len(b);
      const float ub = utt_weights ? utt_weights[b] : 1.f;
      for (int t = 0; t < L; t++) {
        const float w = deriv_weights ? ub * deriv_weights[(size_t)b * T + t] : ub;
        if (w == 1.f) continue;
        float* g = grad + ((size_t)b * T + t) * D;
        if (w == 0.f) { for (int n = 0; n < D; n++) g[n] = 0.f; }
        else { for (int n = 0; n < D; n++) g[n] = g[n] * w; }
      }
    });
  }
  if (sums) {
    double lf = 0.0, sx = 0.0, s2 = 0.0, so = 0.0, sl = 0.0;
    for (int b = 0; b < B; b++) {
      const float u = utt_weights ? utt_weights[b] : 1.f;
      if (u == 0.f) continue;                      // skipped, not multiplied: its objective may be -inf or a NaN
      const double ud = (double)u;
      lf += ud * ((double)den_objf_per_seq[b] - (double)num_objf_per_seq[b]);
      if (xent_objf_per_seq) sx += ud * (double)xent_objf_per_seq[b];
      if (reg_per_seq) { s2 += ud * (double)reg_per_seq[2 * b]; so += ud * (double)reg_per_seq[2 * b + 1]; }
      sl += ud * (double)len(b);
    }
    double v = lf;
    if (xent_objf_per_seq) v += (double)xent_coef * sx;
    if (reg_per_seq) v += (l2 != 0.f ? 0.5 * (double)l2 * s2 : 0.0) + (oor != 0.f ? (double)oor * so : 0.0);
    v *= (double)loss_scale;
    if (loss_norm_dev) v /= (double)*loss_norm_dev;
    if (totals) { const float full = (float)v; totals[0] = full; totals[4] = full; totals[1] = (float)sl; totals[3] = (float)lf; }
    if (weighted) { weighted[0] = (float)lf; weighted[1] = (float)sx; weighted[2] = (float)s2; weighted[3] = (float)so; weighted[4] = (float)sl; }
  }
  return PYCHAIN_HIP_OK;
}

// ---- posterior-target supervision (include/pychain_hip.h: pychain_hip_post_targets, pychain_hip_topk_rows; the device's
// post.hip): the same fp64 sums in the same order of k and frames, the same single fma per addressed gradient element
namespace pychain_hip {
namespace {
inline float post_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
}  // namespace
}  // namespace pychain_hip

extern "C" int pychain_hip_cpu_post_targets(
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, float* grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    const float* den_objf_per_seq, float* num_objf_per_seq, int32_t* bad_count,
    float loss_scale, float* totals, int num_threads) {
  const char* who = "cpu_post_targets";
  if (!nnet_output || !seq_lengths || !target_pdfs || !target_probs || !num_objf_per_seq || !bad_count) return null_pointer(who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  if (totals && !den_objf_per_seq) return fail(PYCHAIN_HIP_EINVAL, "%s: totals need den_objf_per_seq", who);
  g_cpu_calls++;
  float s = grad_scale_dev ? grad_scale * *grad_scale_dev : grad_scale;
  if (loss_norm_dev) s = s / *loss_norm_dev;
  std::vector<double> sums((size_t)B);
  std::vector<int> bads((size_t)B);
  for_each_sequence(B, num_threads, [&](int b) {
    const int L = clamped_length(seq_lengths[b], T);
    double seq = 0.0;
    int bad = 0;
    for (int t = 0; t < L; t++) {
      const size_t f = (size_t)b * T + t;
      const int32_t* pd = target_pdfs + f * K;
      const float* pr = target_probs + f * K;
      const float* x = nnet_output + f * D;
      double acc = 0.0;
      for (int k = 0; k < K; k++) {
        const int d = pd[k];
        if (d < 0) continue;
        if (d >= D) { bad++; continue; }
        const double xd = (double)x[d];
        const double c = xd < -30.0 ? -30.0 : (xd > 30.0 ? 30.0 : xd);
        acc = std::fma((double)pr[k], c, acc);
        if (grad) {
          bool first = true;
          for (int j = 0; j < k; j++) first = first && pd[j] != d;
          if (first) {
            float qd = pr[k];
            for (int j = k + 1; j < K; j++)
              if (pd[j] == d) qd = post_add(qd, pr[j]);
            float* g = grad + f * D + d;
            *g = std::fma(s, qd, *g);
          }
        }
      }
      seq += acc;
    }
    sums[b] = seq; bads[b] = bad;
    num_objf_per_seq[b] = (float)seq;
  });
  int bad = 0;
  for (int b = 0; b < B; b++) bad += bads[b];
  *bad_count = bad;
  if (totals) {
    double sd = 0.0, sn = 0.0;
    for (int b = 0; b < B; b++) { sd += (double)den_objf_per_seq[b]; sn += sums[b]; }
    const double S = sd - sn;
    double v = (double)loss_scale * S;
    if (loss_norm_dev) v /= (double)*loss_norm_dev;
    const float full = (float)v;
    totals[0] = full; totals[4] = full;
    totals[3] = (float)S;
    totals[2] = totals[2] + (float)bad;
  }
  return PYCHAIN_HIP_OK;
}

// ---- sparse entries as cross-entropy targets of z (include/pychain_hip.h: pychain_hip_xent_targets; the device's xent.hip, sparse
// source): qd by the same first-occurrence rule in fp32, everything else - maximum, log-sum-exp, the frame value, the sums - fp64
extern "C" int pychain_hip_cpu_xent_targets(
    const float* z, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, float* xent_grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    float* xent_objf_per_seq, int32_t* bad_count, int num_threads) {
  const char* who = "cpu_xent_targets";
  if (!z || !seq_lengths || !target_pdfs || !target_probs || !xent_objf_per_seq || !bad_count) return null_pointer(who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  g_cpu_calls++;
  float sc = grad_scale_dev ? grad_scale * *grad_scale_dev : grad_scale;
  if (loss_norm_dev) sc = sc / *loss_norm_dev;
  std::vector<int> bads((size_t)B);
  for_each_sequence(B, num_threads, [&](int b) {
    const int L = clamped_length(seq_lengths[b], T);
    if (xent_grad) std::fill(xent_grad + (size_t)b * T * D, xent_grad + (size_t)(b + 1) * T * D, 0.f);
    std::vector<int> pdf_of((size_t)K);               // the frame's distinct live pdfs, where each occurs first, and their qd
    std::vector<float> qd_of((size_t)K);
    double seq = 0.0;
    int bad = 0;
    for (int t = 0; t < L; t++) {
      const size_t f = (size_t)b * T + t;
      const int32_t* pd = target_pdfs + f * K;
      const float* pr = target_probs + f * K;
      int n = 0, nlive = 0;
      for (int k = 0; k < K; k++) {
        const int d = pd[k];
        if (d < 0) continue;
        if (d >= D) { bad++; continue; }
        nlive++;
        bool first = true;
        for (int j = 0; j < k; j++) first = first && pd[j] != d;
        if (!first) continue;
        float qd = pr[k];
        for (int j = k + 1; j < K; j++)
          if (pd[j] == d) qd = post_add(qd, pr[j]);
        pdf_of[n] = d; qd_of[n] = qd; n++;
      }
      if (nlive == 0) continue;                       // no objective, a zero row, and the row of z is not read
      const float* zr = z + f * D;
      double m = -std::numeric_limits<double>::infinity(), se = 0.0, s = 0.0, dot = 0.0;
      for (int d = 0; d < D; d++) if ((double)zr[d] > m) m = (double)zr[d];          // (a NaN is passed by here and met by the sum)
      for (int d = 0; d < D; d++) se += std::exp((double)zr[d] - m);
      for (int i = 0; i < n; i++) { s += (double)qd_of[i]; dot += (double)qd_of[i] * (double)zr[pdf_of[i]]; }
      const double lse = m + std::log(se);
      seq += dot - s * lse;
      if (xent_grad) {
        float* o = xent_grad + f * D;
        std::vector<double> row((size_t)D);
        for (int d = 0; d < D; d++) row[d] = -(s * std::exp((double)zr[d] - lse));
        for (int i = 0; i < n; i++) row[pdf_of[i]] += (double)qd_of[i];
        for (int d = 0; d < D; d++) o[d] = (float)((double)sc * row[d]);
      }
    }
    bads[b] = bad;
    xent_objf_per_seq[b] = (float)seq;
  });
  int bad = 0;
  for (int b = 0; b < B; b++) bad += bads[b];
  *bad_count = bad;
  return PYCHAIN_HIP_OK;
}

// ---- boosted denominator rows (include/pychain_hip.h: pychain_hip_boost_rows; the device's boost.hip): the same fp32 operation
// sequence - clamp, the rounded product with fp32(log2 e), exp2; u = boost qd, the factor by the same two steps, ONE multiply -
// with the host's exp2f where the device has v_exp_f32
namespace pychain_hip {
namespace {
inline float boost_exp(float c) {                       // device_utils.h: exp_bounded
#pragma clang fp contract(off)
  const float t = c * 1.44269502162933349609375f;
  return std::exp2(t);
}
inline float boost_clamp_exp(float v) {                 // (v_med3_f32 turns a NaN into -30)
  const float c = v != v ? -30.f : (v < -30.f ? -30.f : (v > 30.f ? 30.f : v));
  return boost_exp(c);
}
inline float boost_scaled(float E, float boost, float qd) {
#pragma clang fp contract(off)
  const float u = boost * qd;
  const float F = boost_exp(-u);
  return E * F;
}
}  // namespace
}  // namespace pychain_hip

extern "C" int pychain_hip_cpu_boost_rows(
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, float boost,
    float* e, int32_t* bad_count, int num_threads) {
  const char* who = "cpu_boost_rows";
  if (!nnet_output || !seq_lengths || !target_pdfs || !target_probs || !e || !bad_count) return null_pointer(who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  if (!(boost >= 0.f) || !std::isfinite(boost)) return fail(PYCHAIN_HIP_EINVAL, "%s: boost must be finite and not negative, got %g", who, (double)boost);
  g_cpu_calls++;
  std::vector<int> bads((size_t)B);
  for_each_sequence(B, num_threads, [&](int b) {
    const int L = clamped_length(seq_lengths[b], T);
    int bad = 0;
    for (int t = 0; t < L; t++) {
      const size_t f = (size_t)b * T + t;
      const int32_t* pd = target_pdfs + f * K;
      const float* pr = target_probs + f * K;
      const float* x = nnet_output + f * D;
      float* o = e + f * D;
      bool nan = false;
      for (int n = 0; n < D; n++) { nan = nan || x[n] != x[n]; o[n] = boost_clamp_exp(x[n]); }
      if (nan) bad++;
      for (int k = 0; k < K; k++) {
        const int d = pd[k];
        if (d < 0) continue;
        if (d >= D) { bad++; continue; }
        bool first = true;
        for (int j = 0; j < k; j++) first = first && pd[j] != d;
        if (!first) continue;
        float qd = pr[k];
        for (int j = k + 1; j < K; j++)
          if (pd[j] == d) qd = post_add(qd, pr[j]);
        o[d] = boost_scaled(boost_clamp_exp(x[d]), boost, qd);
      }
    }
    bads[b] = bad;
  });
  int bad = 0;
  for (int b = 0; b < B; b++) bad += bads[b];
  *bad_count = bad;
  return PYCHAIN_HIP_OK;
}

extern "C" int pychain_hip_cpu_topk_rows(const float* rows, const int64_t* seq_lengths, int B, int T, int D, int K, float floor,
                                         int normalize, int32_t* out_pdfs, float* out_probs, int num_threads) {
  const char* who = "cpu_topk_rows";
  if (!rows || !seq_lengths || !out_pdfs || !out_probs) return null_pointer(who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1 || K > D || K > 64) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be in [1, min(D, 64)], got %d (D = %d)", who, K, D);
  g_cpu_calls++;
  for_each_sequence(B, num_threads, [&](int b) {
    const int L = clamped_length(seq_lengths[b], T);
    for (int t = 0; t < T; t++) {
      const size_t f = (size_t)b * T + t;
      int32_t* op = out_pdfs + f * K;
      float* ov = out_probs + f * K;
      int n = 0;
      if (t < L) {
        const float* r = rows + f * D;
        float lastv = 0.f;
        int lasti = -1;
        for (; n < K; n++) {                       // the next element behind the previous pick: value descending, index ascending
          int bi = -1;
          float bv = 0.f;
          for (int i = 0; i < D; i++) {
            const float v = r[i];
            const bool ok = v >= floor && (lasti < 0 || v < lastv || (v == lastv && i > lasti));
            if (ok && (bi < 0 || v > bv)) { bv = v; bi = i; }
          }
          if (bi < 0) break;
          op[n] = bi; ov[n] = bv;
          lastv = bv; lasti = bi;
        }
        if (normalize && n > 0) {
          float sum = 0.f;
          for (int j = 0; j < n; j++) sum = post_add(sum, ov[j]);
          for (int j = 0; j < n; j++) ov[j] = ov[j] / sum;
        }
      }
      for (int j = n; j < K; j++) { op[j] = -1; ov[j] = 0.f; }
    }
  });
  return PYCHAIN_HIP_OK;
}

// ---- lattice-free sMBR (include/pychain_hip.h: pychain_hip_smbr_*; the device's smbr.hip): the same equations
// on host pointers - fp32 state vectors and gradient, fp64 sums; the accuracies centred by the frame accuracies of the first call.
// With a class map (pychain_hip_cpu_smbr_*_classes) the accuracy row is dense, A(t,n) = Acls(t, cls[n]), and the
// gradient row is centred by its own mean, as the device's smbr_class_grad_kernel does.
namespace pychain_hip {
namespace {
// the frame's accuracy of pdf d: the sum of its entries' q, in ascending k
inline float smbr_accuracy(const int32_t* pd, const float* pr, int K, int d) {
  float q = 0.f;
  for (int k = 0; k < K; k++)
    if (pd[k] == d) q = post_add(q, pr[k]);
  return q;
}

// accuracy by class: the class of a target id, -1 where it adds nothing; Acls(t, .) of a frame, q summed in
// ascending k
struct SmbrHostClasses { const int32_t* cls; int C; bool targets_are_classes; };
inline int smbr_entry_class(const SmbrHostClasses& c, int id, int D) {
  if (id < 0) return -1;
  if (c.targets_are_classes) return id < c.C ? id : -1;
  return id < D ? c.cls[id] : -1;
}
inline void smbr_class_table(const SmbrHostClasses& c, const int32_t* pd, const float* pr, int K, int D, float* acl) {
  for (int i = 0; i < c.C; i++) acl[i] = 0.f;
  for (int k = 0; k < K; k++) {
    const int cc = smbr_entry_class(c, pd[k], D);
    if (cc >= 0 && cc < c.C) acl[cc] = post_add(acl[cc], pr[k]);
  }
}

bool smbr_one(const Csr& fwd, const Csr& bwd, const float* leaky, const float* init, const float* fin, const int32_t* parc, const int32_t* pidx,
              int H, const float* x, int L, int D, const int32_t* pdfs, const float* probs, int K, const float* facc, float coef,
              float gscale, float* grad, float* closing, const SmbrHostClasses* cls = nullptr) {
  const size_t rows = (size_t)L + 1;
  std::vector<float> al(rows * H), ab(rows * H, 0.f), be(rows * H), bb(rows * H, 0.f), xr((size_t)D), xa((size_t)D);
  std::vector<float> acl(cls ? (size_t)cls->C : 0);
  bool ok = true, den_ok = true;                   // what the recursions find; what the gradient frames find
  auto stage = [&](int t) {                        // x = exp(clamp(y)) and its companion x A: sparse, or dense by class
    const float* y = x + (size_t)t * D;
    for (int n = 0; n < D; n++) {
      if (y[n] != y[n]) ok = false;
      xr[n] = std::exp(y[n] != y[n] ? -30.f : clamp30(y[n]));
      xa[n] = 0.f;
    }
    if (cls) {
      smbr_class_table(*cls, pdfs + (size_t)t * K, probs + (size_t)t * K, K, D, acl.data());
      for (int n = 0; n < D; n++) {
        const int cc = cls->cls[n];
        xa[n] = cc >= 0 && cc < cls->C ? xr[n] * acl[cc] : 0.f;
      }
      return;
    }
    for (int k = 0; k < K; k++) {
      const int d = pdfs[(size_t)t * K + k];
      if (d >= 0 && d < D) xa[d] = xr[d] * smbr_accuracy(pdfs + (size_t)t * K, probs + (size_t)t * K, K, d);
    }
  };
  auto positive = [&](double tot) { if (!(tot > 0.0) || !std::isfinite(tot) || !std::isfinite(1.0 / tot)) ok = false; };
  {
    double tot = 0.0;
    for (int i = 0; i < H; i++) tot += (double)init[i];
    positive(tot);
    for (int i = 0; i < H; i++) al[i] = (float)((double)init[i] / tot + (double)coef * leaky[i]);
  }
  std::vector<double> r0((size_t)H), r1((size_t)H);
  for (int t = 0; t < L; t++) {
    stage(t);
    const float *a0 = al.data() + (size_t)t * H, *a1 = ab.data() + (size_t)t * H;
    double tot = 0.0, s1 = 0.0;
    for (int j = 0; j < H; j++) {
      double acc0 = 0.0, acc1 = 0.0;
      for (int k = bwd.idx[2 * j]; k < bwd.idx[2 * j + 1]; k++) {
        const int src = bwd.trans[3 * k], n = bwd.trans[3 * k + 2];
        const double wu = (double)bwd.prob[k] * a0[src];
        acc0 += wu * xr[n];
        acc1 += (double)bwd.prob[k] * a1[src] * xr[n] + wu * xa[n];
      }
      acc1 -= (double)facc[t] * acc0;
      r0[j] = acc0; r1[j] = acc1;
      tot += acc0; s1 += acc1;
    }
    positive(tot);
    float *o0 = al.data() + (size_t)(t + 1) * H, *o1 = ab.data() + (size_t)(t + 1) * H;
    for (int j = 0; j < H; j++) {
      const double lk = (double)coef * leaky[j];
      o0[j] = (float)(r0[j] / tot + lk);
      o1[j] = (float)((r1[j] + lk * s1) / tot);
    }
  }
  {
    double tot = 0.0, w = 0.0;
    for (int i = 0; i < H; i++) { tot += (double)fin[i]; w += (double)fin[i] * leaky[i]; }
    positive(tot);
    for (int i = 0; i < H; i++) be[(size_t)L * H + i] = (float)(((double)fin[i] + (double)coef * w) / tot);
  }
  for (int t = L - 1; t >= 0; t--) {
    stage(t);
    const float *b0 = be.data() + (size_t)(t + 1) * H, *b1 = bb.data() + (size_t)(t + 1) * H;
    double tot = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < H; i++) {
      double acc0 = 0.0, acc1 = 0.0;
      for (int k = fwd.idx[2 * i]; k < fwd.idx[2 * i + 1]; k++) {
        const int dst = fwd.trans[3 * k + 1], n = fwd.trans[3 * k + 2];
        const double wu = (double)fwd.prob[k] * b0[dst];
        acc0 += wu * xr[n];
        acc1 += (double)fwd.prob[k] * b1[dst] * xr[n] + wu * xa[n];
      }
      acc1 -= (double)facc[t] * acc0;
      r0[i] = acc0; r1[i] = acc1;
      tot += acc0; s1 += acc0 * leaky[i]; s2 += acc1 * leaky[i];
    }
    positive(tot);
    float *o0 = be.data() + (size_t)t * H, *o1 = bb.data() + (size_t)t * H;
    for (int i = 0; i < H; i++) {
      o0[i] = (float)((r0[i] + (double)coef * s1) / tot);
      o1[i] = (float)((r1[i] + (double)coef * s2) / tot);
    }
    // the gradient of frame t: alpha'(t), alpha-bar'(t), beta'(t+1), beta-bar'(t+1); x and x A of frame t are staged
    const float *a0 = al.data() + (size_t)t * H, *a1 = ab.data() + (size_t)t * H;
    std::vector<double> v((size_t)D), u((size_t)D, 0.0);
    double den = 0.0, mean = 0.0;
    for (int n = 0; n < D; n++) {
      double q0 = 0.0, q1 = 0.0;
      for (int k = pidx[n]; k < pidx[n + 1]; k++) {
        const int id = parc[k], src = fwd.trans[3 * id], dst = fwd.trans[3 * id + 1];
        const double wa = (double)fwd.prob[id] * a0[src];
        q0 += wa * b0[dst];
        q1 += (double)fwd.prob[id] * a1[src] * b0[dst] + wa * b1[dst];
      }
      if (pidx[n] == pidx[n + 1]) { v[n] = 0.0; continue; }
      v[n] = (double)xr[n] * (q1 - (double)facc[t] * q0) + (double)xa[n] * q0;
      u[n] = (double)xr[n] * q0;
      den += u[n];
      mean += v[n];
    }
    // the frame's divisor, as the device checks it: it decides the verdict, not `closing` (a diagnostic of the recursions)
    if (!(den > 0.0) || !std::isfinite(den) || !std::isfinite(1.0 / den)) den_ok = false;
    float* go = grad + (size_t)t * D;
    // The row is centred by its own mean, in both forms, as the device does (smbr.hip: smbr_grad_kernel, smbr_class_grad_kernel).
    // sum_n v is zero but for the rounding of e(t) - the occupancies are stage 1's, in fp32 -, and that residue enters alpha-bar
    // and beta-bar at every frame and stays: uncentred, a row carries gamma(t,n) times the residue ACCUMULATED over the sequence
    // (`closing` is that sum): 3e-2 of max |grad| at 1500 frames here, where stage 1's occupancies are the host's.
    const double eps = mean / den;
    for (int n = 0; n < D; n++) go[n] = pidx[n] == pidx[n + 1] ? 0.f : (float)((double)gscale * (v[n] - eps * u[n]) / den);
  }
  double c0 = 0.0, c1 = 0.0;
  for (int i = 0; i < H; i++) { c0 += (double)al[(size_t)L * H + i] * fin[i]; c1 += (double)ab[(size_t)L * H + i] * fin[i]; }
  if (!(c0 > 0.0)) ok = false;
  *closing = ok ? (float)(c1 / c0) : std::numeric_limits<float>::quiet_NaN();
  return ok && den_ok;
}
}  // namespace
}  // namespace pychain_hip

namespace {
int cpu_smbr_frame_accuracy(const char* who, const float* gamma, const int64_t* seq_lengths, int B, int T, int D,
                            const int32_t* target_pdfs, const float* target_probs, int K,
                            float* frame_acc, double* acc_per_seq, int32_t* bad_count, int num_threads, const SmbrHostClasses* cls) {
  if (!gamma || !seq_lengths || !target_pdfs || !target_probs || !frame_acc || !acc_per_seq || !bad_count) return null_pointer(who);
  if (B <= 0 || T <= 0 || D <= 0) return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d D=%d", who, B, T, D);
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  g_cpu_calls++;
  std::vector<int> bads((size_t)B);
  for_each_sequence(B, num_threads, [&](int b) {
    const int L = clamped_length(seq_lengths[b], T);
    double sum = 0.0;
    int bad = 0;
    std::vector<float> acl(cls ? (size_t)cls->C : 0);
    for (int t = 0; t < L; t++) {
      const size_t f = (size_t)b * T + t;
      double e = 0.0;
      if (cls) {                                   // e = sum_n gamma(n) Acls(cls[n]), ascending n
        for (int k = 0; k < K; k++)
          if (target_pdfs[f * K + k] >= (cls->targets_are_classes ? cls->C : D)) bad++;
        smbr_class_table(*cls, target_pdfs + f * K, target_probs + f * K, K, D, acl.data());
        for (int n = 0; n < D; n++) {
          const int cc = cls->cls[n];
          if (cc >= 0 && cc < cls->C) e += (double)gamma[f * D + n] * (double)acl[cc];
        }
      }
      for (int k = 0; k < K && !cls; k++) {
        const int d = target_pdfs[f * K + k];
        if (d < 0) continue;
        if (d >= D) { bad++; continue; }
        e += (double)target_probs[f * K + k] * (double)gamma[f * D + d];
      }
      frame_acc[f] = (float)e;
      sum += e;
    }
    acc_per_seq[b] = sum;
    bads[b] = bad;
  });
  bad_count[0] = bad_count[1] = 0;
  for (int b = 0; b < B; b++) bad_count[1] += bads[b];
  return PYCHAIN_HIP_OK;
}
int cpu_bad_classes(const char* who, const int32_t* pdf_classes, int num_classes, int targets_are_classes) {
  if (!pdf_classes && targets_are_classes) return fail(PYCHAIN_HIP_EINVAL, "%s: targets_are_classes needs pdf_classes", who);
  if (pdf_classes && num_classes < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: num_classes must be at least 1 with pdf_classes, got %d", who, num_classes);
  return PYCHAIN_HIP_OK;
}
}  // namespace

extern "C" int pychain_hip_cpu_smbr_frame_accuracy(const float* gamma, const int64_t* seq_lengths, int B, int T, int D,
                                                   const int32_t* target_pdfs, const float* target_probs, int K,
                                                   float* frame_acc, double* acc_per_seq, int32_t* bad_count, int num_threads) {
  return cpu_smbr_frame_accuracy("cpu_smbr_frame_accuracy", gamma, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc, acc_per_seq,
                                 bad_count, num_threads, nullptr);
}

extern "C" int pychain_hip_cpu_smbr_frame_accuracy_classes(const float* gamma, const int64_t* seq_lengths, int B, int T, int D,
                                                           const int32_t* target_pdfs, const float* target_probs, int K,
                                                           float* frame_acc, double* acc_per_seq, int32_t* bad_count, int num_threads,
                                                           const int32_t* pdf_classes, int num_classes, int targets_are_classes) {
  const char* who = pdf_classes ? "cpu_smbr_frame_accuracy_classes" : "cpu_smbr_frame_accuracy";
  const int rc = cpu_bad_classes("cpu_smbr_frame_accuracy_classes", pdf_classes, num_classes, targets_are_classes);
  if (rc != PYCHAIN_HIP_OK) return rc;
  const SmbrHostClasses c{pdf_classes, num_classes, targets_are_classes != 0};
  return cpu_smbr_frame_accuracy(who, gamma, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc, acc_per_seq, bad_count, num_threads,
                                 pdf_classes ? &c : nullptr);
}

namespace {
int cpu_smbr_forward_backward(
    const char* who,
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    float* grad, double* acc_per_seq, float* closing, int32_t* bad_count, int num_threads, const SmbrHostClasses* cls) {
  const NumGraphs g{ft, fi, fp, bt, bi, bp, initial, final_, 0, H, num_arcs};
  if (g.any_null() || !leaky || !pdf_arcs || !pdf_index || !nnet_output || !seq_lengths || !target_pdfs || !target_probs || !frame_acc ||
      !grad || !acc_per_seq || !closing || !bad_count)
    return null_pointer(who);
  int rc = bad_sizes(who, B, T, H, num_arcs, D);
  if (rc != PYCHAIN_HIP_OK) return rc;
  if (K < 1) return fail(PYCHAIN_HIP_EINVAL, "%s: K must be at least 1, got %d", who, K);
  if (!(leaky_hmm_coefficient > 0.f && leaky_hmm_coefficient < 1.f))
    return fail(PYCHAIN_HIP_EINVAL, "%s: leaky_hmm_coefficient must be in (0,1), got %g", who, (double)leaky_hmm_coefficient);
  g_cpu_calls++;
  const float gscale = grad_scale * (grad_scale_dev ? *grad_scale_dev : 1.f);
  std::atomic<int> bad{0};
  for_each_sequence(B, num_threads, [&](int b) {
    const int L = clamped_length(seq_lengths[b], T);
    const size_t f = (size_t)b * T;
    float* gb = grad + f * D;
    const bool ok = smbr_one(fwd_of(g), bwd_of(g), leaky, initial, final_, pdf_arcs, pdf_index, H, nnet_output + f * D, L, D,
                             target_pdfs + f * K, target_probs + f * K, K, frame_acc + f, leaky_hmm_coefficient, gscale, gb, closing + b, cls);
    for (size_t i = (size_t)L * D; i < (size_t)T * D; i++) gb[i] = 0.f;
    if (!ok) { bad++; acc_per_seq[b] = std::numeric_limits<double>::quiet_NaN(); }
  });
  bad_count[0] += bad.load();
  return PYCHAIN_HIP_OK;
}
}  // namespace

extern "C" int pychain_hip_cpu_smbr_forward_backward(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    float* grad, double* acc_per_seq, float* closing, int32_t* bad_count, int num_threads) {
  return cpu_smbr_forward_backward("cpu_smbr_forward_backward", ft, fi, fp, bt, bi, bp, leaky, initial, final_, pdf_arcs, pdf_index, H, num_arcs,
                                   nnet_output, seq_lengths, B, T, D, target_pdfs, target_probs, K, frame_acc, leaky_hmm_coefficient, grad_scale,
                                   grad_scale_dev, grad, acc_per_seq, closing, bad_count, num_threads, nullptr);
}

extern "C" int pychain_hip_cpu_smbr_forward_backward_classes(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    float* grad, double* acc_per_seq, float* closing, int32_t* bad_count, int num_threads,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes) {
  const int rc = cpu_bad_classes("cpu_smbr_forward_backward_classes", pdf_classes, num_classes, targets_are_classes);
  if (rc != PYCHAIN_HIP_OK) return rc;
  const SmbrHostClasses c{pdf_classes, num_classes, targets_are_classes != 0};
  return cpu_smbr_forward_backward(pdf_classes ? "cpu_smbr_forward_backward_classes" : "cpu_smbr_forward_backward", ft, fi, fp, bt, bi, bp, leaky,
                                   initial, final_, pdf_arcs, pdf_index, H, num_arcs, nnet_output, seq_lengths, B, T, D, target_pdfs, target_probs,
                                   K, frame_acc, leaky_hmm_coefficient, grad_scale, grad_scale_dev, grad, acc_per_seq, closing, bad_count,
                                   num_threads, pdf_classes ? &c : nullptr);
}

// ---- expected arc counts (include/pychain_hip.h: pychain_hip_den_arc_counts; the device: arc_counts.hip) -----------
// The same equations with fp32 state vectors, every sum in fp64, and the sequences dealt to host threads: the plain alpha' / beta'
// recursions of smbr_one over p exp(w), then per frame the arc posteriors alpha'(t,src) p e^w x(t,pdf) beta'(t+1,dst) / (their
// sum), added to the sequence's counts and, by pdf, into the gradient row.
namespace pychain_hip {
namespace {
bool arc_counts_one(const Csr& fwd, const Csr& bwd, const float* pwf, const float* pwb, const float* leaky, const float* init, const float* fin,
                    const int32_t* parc, const int32_t* pidx, int H, const float* x, int L, int D, float coef, float gscale,
                    float* grad, double* counts, double* objf) {
  const size_t rows = (size_t)L + 1;
  std::vector<float> al(rows * H), be(rows * H), xr((size_t)D);
  std::vector<double> r0((size_t)H);
  bool ok = true;
  auto stage = [&](int t) {
    const float* y = x + (size_t)t * D;
    for (int n = 0; n < D; n++) {
      if (y[n] != y[n]) ok = false;
      xr[n] = std::exp(y[n] != y[n] ? -30.f : clamp30(y[n]));
    }
  };
  auto positive = [&](double tot) { if (!(tot > 0.0) || !std::isfinite(tot) || !std::isfinite(1.0 / tot)) ok = false; };
  double lz = 0.0;
  {
    double tot = 0.0;
    for (int i = 0; i < H; i++) tot += (double)init[i];
    positive(tot);
    lz += std::log(tot);
    for (int i = 0; i < H; i++) al[i] = (float)((double)init[i] / tot + (double)coef * leaky[i]);
  }
  for (int t = 0; t < L; t++) {
    stage(t);
    const float* a0 = al.data() + (size_t)t * H;
    double tot = 0.0;
    for (int j = 0; j < H; j++) {
      double acc = 0.0;
      for (int k = bwd.idx[2 * j]; k < bwd.idx[2 * j + 1]; k++) acc += (double)pwb[k] * a0[bwd.trans[3 * k]] * xr[bwd.trans[3 * k + 2]];
      r0[j] = acc; tot += acc;
    }
    positive(tot);
    lz += std::log(tot);
    float* o0 = al.data() + (size_t)(t + 1) * H;
    for (int j = 0; j < H; j++) o0[j] = (float)(r0[j] / tot + (double)coef * leaky[j]);
  }
  {
    double tot = 0.0, w = 0.0, c0 = 0.0;
    for (int i = 0; i < H; i++) { tot += (double)fin[i]; w += (double)fin[i] * leaky[i]; c0 += (double)al[(size_t)L * H + i] * fin[i]; }
    positive(tot);
    if (!(c0 > 0.0)) ok = false;
    lz += std::log(c0);
    for (int i = 0; i < H; i++) be[(size_t)L * H + i] = (float)(((double)fin[i] + (double)coef * w) / tot);
  }
  for (int t = L - 1; t >= 0; t--) {
    stage(t);
    const float* b0 = be.data() + (size_t)(t + 1) * H;
    double tot = 0.0, s1 = 0.0;
    for (int i = 0; i < H; i++) {
      double acc = 0.0;
      for (int k = fwd.idx[2 * i]; k < fwd.idx[2 * i + 1]; k++) acc += (double)pwf[k] * b0[fwd.trans[3 * k + 1]] * xr[fwd.trans[3 * k + 2]];
      r0[i] = acc; tot += acc; s1 += acc * leaky[i];
    }
    positive(tot);
    float* o0 = be.data() + (size_t)t * H;
    for (int i = 0; i < H; i++) o0[i] = (float)((r0[i] + (double)coef * s1) / tot);
    // the arc posteriors of frame t: alpha'(t), beta'(t+1); x of frame t is staged
    const float* a0 = al.data() + (size_t)t * H;
    double den = 0.0;
    for (int n = 0; n < D; n++)
      for (int k = pidx[n]; k < pidx[n + 1]; k++) {
        const int id = parc[k];
        den += (double)pwf[id] * a0[fwd.trans[3 * id]] * b0[fwd.trans[3 * id + 1]] * xr[n];
      }
    if (!(den > 0.0) || !std::isfinite(den) || !std::isfinite(1.0 / den)) ok = false;
    for (int n = 0; n < D; n++) {
      double g = 0.0;
      for (int k = pidx[n]; k < pidx[n + 1]; k++) {
        const int id = parc[k];
        const double post = (double)pwf[id] * a0[fwd.trans[3 * id]] * b0[fwd.trans[3 * id + 1]] * xr[n] / den;
        counts[id] += post;
        g += post;
      }
      if (grad) grad[(size_t)t * D + n] = pidx[n] == pidx[n + 1] ? 0.f : (float)((double)gscale * g);
    }
  }
  if (!std::isfinite(lz)) ok = false;
  *objf = lz;
  return ok;
}
}  // namespace
}  // namespace pychain_hip

extern "C" int pychain_hip_cpu_den_arc_counts(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* leaky, const float* initial, const float* final_, const int32_t* pdf_arcs, const int32_t* pdf_index, int H, int num_arcs,
    const float* arc_log_weights, const float* nnet_output, const int64_t* seq_lengths, int B, int T, int D,
    float leaky_hmm_coefficient, const float* seq_weights, float grad_scale, const float* grad_scale_dev,
    float* grad, double* objf_per_seq, double* counts, double* counts_per_seq, int32_t* bad_count, int num_threads) {
  const char* who = "cpu_den_arc_counts";
  const NumGraphs g{ft, fi, fp, bt, bi, bp, initial, final_, 0, H, num_arcs};
  if (g.any_null() || !leaky || !pdf_arcs || !pdf_index || !nnet_output || !seq_lengths || !objf_per_seq || !counts || !bad_count)
    return null_pointer(who);
  int rc = bad_sizes(who, B, T, H, num_arcs, D);
  if (rc != PYCHAIN_HIP_OK) return rc;
  if (!(leaky_hmm_coefficient > 0.f && leaky_hmm_coefficient < 1.f))
    return fail(PYCHAIN_HIP_EINVAL, "%s: leaky_hmm_coefficient must be in (0,1), got %g", who, (double)leaky_hmm_coefficient);
  g_cpu_calls++;
  const int K = num_arcs;
  bad_count[0] = bad_count[1] = 0;
  // p exp(w) in both orders: the backward copy of an arc is the r-th arc of its source's run with these endpoints, pdf and
  // probability, r its rank among the equal arcs of its destination's run (arc_counts.hip: arc_weight_kernel)
  std::vector<float> pwf((size_t)K), pwb((size_t)K);
  auto weighted = [&](int id, float p, bool count) {
    if (!arc_log_weights || id < 0) return p;
    const float w = arc_log_weights[id];
    if (!std::isfinite(w)) { if (count) bad_count[1]++; return p; }
    return p * std::exp(w);
  };
  for (int k = 0; k < K; k++) pwf[k] = weighted(k, fp[k], true);
  for (int k = 0; k < K; k++) {
    const int src = bt[3 * k], dst = bt[3 * k + 1], pdf = bt[3 * k + 2];
    int id = -1;
    if (arc_log_weights && src >= 0 && src < H && dst >= 0 && dst < H) {
      int rank = 0;
      for (int j = bi[2 * dst] < 0 ? 0 : bi[2 * dst]; j < k; j++)
        if (bt[3 * j] == src && bt[3 * j + 2] == pdf && bp[j] == bp[k]) rank++;
      const int j1 = fi[2 * src + 1] < K ? fi[2 * src + 1] : K;
      for (int j = fi[2 * src] < 0 ? 0 : fi[2 * src]; j < j1; j++)
        if (ft[3 * j + 1] == dst && ft[3 * j + 2] == pdf && fp[j] == bp[k] && rank-- == 0) { id = j; break; }
    }
    pwb[k] = weighted(id, bp[k], false);
  }
  const float gs = grad_scale * (grad_scale_dev ? *grad_scale_dev : 1.f);
  std::vector<double> per((size_t)B * K, 0.0);
  std::vector<char> bads((size_t)B, 0);
  for_each_sequence(B, num_threads, [&](int b) {
    const int L = clamped_length(seq_lengths[b], T);
    const size_t f = (size_t)b * T;
    float* gb = grad ? grad + f * D : nullptr;
    const float u = seq_weights ? seq_weights[b] : 1.f;
    const bool ok = arc_counts_one(fwd_of(g), bwd_of(g), pwf.data(), pwb.data(), leaky, initial, final_, pdf_arcs, pdf_index, H,
                                   nnet_output + f * D, L, D, leaky_hmm_coefficient, gs * u, gb, per.data() + (size_t)b * K, objf_per_seq + b);
    if (gb) for (size_t i = (size_t)L * D; i < (size_t)T * D; i++) gb[i] = 0.f;
    if (!ok) {
      bads[b] = 1;
      objf_per_seq[b] = std::numeric_limits<double>::quiet_NaN();
      for (int k = 0; k < K; k++) per[(size_t)b * K + k] = 0.0;
    }
  });
  for (int k = 0; k < K; k++) counts[k] = 0.0;
  for (int b = 0; b < B; b++) {                    // in ascending b, whatever thread ran the sequence
    bad_count[0] += bads[b];
    const float u = seq_weights ? seq_weights[b] : 1.f;
    if (!bads[b] && u != 0.f)
      for (int k = 0; k < K; k++) counts[k] += (double)u * per[(size_t)b * K + k];
  }
  if (counts_per_seq) memcpy(counts_per_seq, per.data(), per.size() * sizeof(double));
  return PYCHAIN_HIP_OK;
}
