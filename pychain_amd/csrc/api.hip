// api.hip - the C ABI of libpychain_hip.so (include/pychain_hip.h): argument checks,
// workspace carving, launches.  No allocation, no host synchronisation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "../../include/pychain_hip.h"
#include "call_args.h"
#include "common.h"
#include "den_kernels.h"
#include "den_policy.h"
#include "device_utils.h"
#include "num_arcs.h"
#include "num_kernels.h"
#include "plan_format.h"
#include "xent.h"

namespace pychain_hip {
char* last_error_buffer() {
  static thread_local char buf[512] = "";
  return buf;
}
namespace {
// ---- settings: process-wide defaults + per-thread overrides, snapshotted per call (common.h:CallKnobs) ----------
std::mutex g_option_lock;
typedef std::map<std::string, std::string> OptionTable;
OptionTable& process_options() { static OptionTable t; return t; }
OptionTable& thread_options() { static thread_local OptionTable t; return t; }     // "" = unset for this thread
// every option of the library and what call_knobs() takes where it is unset ("debug_corrupt_row": parsed there; "gamma16": set = on)
struct OptionSpec { const char* name; int dflt; };
const OptionSpec kOptions[] = {{"verbose", 0}, {"den_phase_mask", 3}, {"den_lazy", 1}, {"den_dma", -1}, {"den_segments", 0}, {"den_pair", -1},
                               {"gamma16", 0}, {"debug_corrupt_row", 0}, {"num_compat", 0}, {"den_tseg", -1}, {"den_tburn", 192},
                               {"plan_split", -1}, {"chain_slices", -1}, {"den_sg", 1}, {"den_cross", 0}, {"den_q", 0}, {"num_arcs_gather", 0}};
const OptionSpec* find_option(const char* name) {
  if (!name) return nullptr;
  for (const OptionSpec& o : kOptions) if (strcmp(o.name, name) == 0) return &o;
  return nullptr;
}
bool known_option(const char* name) { return find_option(name) != nullptr; }
// effective value of one option as a COPY (the tables may change under another thread's set_option)
bool option_value(const char* name, std::string* out) {
  const OptionTable& th = thread_options();
  auto it = th.find(name);
  if (it != th.end()) { if (it->second.empty()) return false; *out = it->second; return true; }
  std::lock_guard<std::mutex> guard(g_option_lock);
  const OptionTable& pr = process_options();
  auto ip = pr.find(name);
  if (ip == pr.end()) return false;
  *out = ip->second;
  return true;
}
int option_int(const char* name) {            // (a name of kOptions)
  std::string v;
  return option_value(name, &v) ? atoi(v.c_str()) : find_option(name)->dflt;
}
bool option_set(const char* name) { std::string v; return option_value(name, &v); }
}  // namespace

CallKnobs call_knobs() {
  CallKnobs k;
  memset(&k, 0, sizeof(k));
  k.verbose = option_int("verbose");
  k.den_phase_mask = option_int("den_phase_mask") & 3;
  k.den_lazy = option_int("den_lazy") ? 1 : 0;
  k.den_segments = option_int("den_segments");
  k.gamma16 = option_set("gamma16");
  k.den_pair = option_int("den_pair");
  k.den_dma = option_int("den_dma");
  k.num_compat = option_int("num_compat") ? 1 : 0;
  k.den_tseg = option_int("den_tseg");
  k.den_tburn = option_int("den_tburn");
  k.plan_split = option_int("plan_split");
  k.chain_slices = option_int("chain_slices");
  k.den_sg = option_int("den_sg") ? 1 : 0;
  k.den_q = option_int("den_q") ? 1 : 0;          // (off by default: the frame is bound by VALU issue, not by the LDS time it saves - DESIGN.md 3.16)
  k.num_arcs_gather = option_int("num_arcs_gather") ? 1 : 0;   // (test aid: the gathered form of num_arc_count_kernel where the staged one fits - DESIGN.md 3.31)
  k.den_cross = option_int("den_cross") ? 1 : 0;   // (off by default: measured slower than the streamed occupancy launch - DESIGN.md 3.15)
  std::string v;
  if (option_value("debug_corrupt_row", &v)) {   // "den,b,t,scale" / "num,b,t,scale"
    char what[8] = ""; int b = 0, t = 0; float sc = 1.f;
    if (sscanf(v.c_str(), "%3[a-z],%d,%d,%f", what, &b, &t, &sc) == 4 && b >= 0 && t >= 0) {
      k.corrupt_what = strcmp(what, "den") == 0 ? 1 : (strcmp(what, "num") == 0 ? 2 : 0);
      k.corrupt_b = b; k.corrupt_t = t; k.corrupt_scale = sc;
    }
  }
  return k;
}
}  // namespace pychain_hip

using namespace pychain_hip;

extern "C" int pychain_hip_abi_version(void) { return PYCHAIN_HIP_ABI_VERSION; }
extern "C" const char* pychain_hip_last_error(void) { return last_error_buffer(); }
extern "C" int pychain_hip_set_option(const char* name, const char* value) {
  if (!known_option(name)) return fail(PYCHAIN_HIP_EINVAL, "set_option: unknown option '%s'", name ? name : "(null)");
  std::lock_guard<std::mutex> guard(g_option_lock);
  if (value && *value) process_options()[name] = value; else process_options().erase(name);
  return PYCHAIN_HIP_OK;
}
extern "C" int pychain_hip_set_thread_option(const char* name, const char* value) {
  if (!known_option(name)) return fail(PYCHAIN_HIP_EINVAL, "set_thread_option: unknown option '%s'", name ? name : "(null)");
  if (value) thread_options()[name] = value; else thread_options().erase(name);
  return PYCHAIN_HIP_OK;
}
extern "C" int pychain_hip_get_option(const char* name, char* buf, size_t buf_bytes) {
  if (!known_option(name)) return fail(PYCHAIN_HIP_EINVAL, "get_option: unknown option '%s'", name ? name : "(null)");
  std::string v;
  if (!option_value(name, &v)) return 0;
  if (buf && buf_bytes > 0) { strncpy(buf, v.c_str(), buf_bytes - 1); buf[buf_bytes - 1] = 0; }
  return (int)v.size();
}
static void set_process_int(const char* name, int v) {
  char s[32];
  snprintf(s, sizeof(s), "%d", v);
  pychain_hip_set_option(name, s);
}
extern "C" void pychain_hip_set_verbose_level(int level) { set_process_int("verbose", level); }
extern "C" int pychain_hip_get_verbose_level(void) { return call_knobs().verbose; }
extern "C" void pychain_hip_set_den_phase_mask(int mask) { set_process_int("den_phase_mask", mask & 3); }
extern "C" void pychain_hip_set_den_lazy(int on) { set_process_int("den_lazy", on ? 1 : 0); }

extern "C" int pychain_hip_den_kernel_names(int hint, int H, int D, int B, int plans_shared,
                                            char* buf, size_t buf_bytes) {
  if (!buf || buf_bytes == 0 || H <= 0 || D <= 0 || B <= 0) return fail(PYCHAIN_HIP_EINVAL, "den_kernel_names: bad arguments");
  if (hint == PYCHAIN_HIP_HINT_GENERAL) {
    snprintf(buf, buf_bytes, "den_general_recursion_kernel,den_general_gamma_kernel");
    return PYCHAIN_HIP_OK;
  }
  // (the names of a call of the denominator alone that evaluates both launches, of sequences long enough to have two halves: the
  // crossing where option den_cross asks for it; plans_shared bit 1: the call is a fused loss)
  DenArgs a = den_query_args((plans_shared & 1) ? 0 : 256, hint, H, D, B, 1 << 14, (plans_shared & 2) != 0);
  a.xf = (a.sg && !a.fused && 2 * a.B <= device_cu_count() && den_xf_eligible(a, hint)) ? den_xf_band() : 0;
  snprintf(buf, buf_bytes, "%s,%s", den_recursion_kernel_name(a, hint),
           den_occupancy_kernel_name(a, (D + 63) / 64, hint));
  return PYCHAIN_HIP_OK;
}

extern "C" int pychain_hip_den_plan_info(const void* host_blob, size_t blob_bytes, int32_t info[8]) {
  if (!host_blob || !info || blob_bytes < sizeof(PlanHeader))
    return fail(PYCHAIN_HIP_EINVAL, "den_plan_info: null or truncated blob");
  if (((const int32_t*)host_blob)[0] == PLAN_MAGIC_GENERAL) {
    const GeneralPlanHeader* gh = (const GeneralPlanHeader*)host_blob;
    if (blob_bytes < sizeof(GeneralPlanHeader) || gh->version != PLAN_VERSION || (size_t)gh->total_bytes > blob_bytes ||
        (size_t)gh->total_bytes < sizeof(GeneralPlanHeader))
      return fail(PYCHAIN_HIP_EINVAL, "den_plan_info: not a plan of this library version");
    if ((int32_t)general_payload_hash(host_blob, (size_t)gh->total_bytes) != gh->payload_hash ||
        (int32_t)general_header_hash(*gh) != gh->reserved[0])
      return fail(PYCHAIN_HIP_EINVAL, "den_plan_info: plan does not match its checksums (corrupted or foreign file)");
    {
      const int64_t n = gh->total_bytes, H8 = (int64_t)gh->H * 8, K8 = (int64_t)gh->K * 8, K4 = (int64_t)gh->K * 4, Hp4 = (int64_t)gh->Hp * 4;
      const int64_t offs[12] = {gh->off_a_idx, gh->off_a_arc, gh->off_a_p, gh->off_b_idx, gh->off_b_arc, gh->off_b_p,
                                gh->off_g_idx, gh->off_g_arc, gh->off_g_p, gh->off_leaky, gh->off_init, gh->off_final};
      const int64_t lens[12] = {H8, K8, K4, H8, K8, K4, ((int64_t)gh->D + 1) * 4, K8, K4, Hp4, Hp4, Hp4};
      for (int i = 0; i < 12; i++)
        if (offs[i] < (int64_t)sizeof(GeneralPlanHeader) || offs[i] + lens[i] > n)
          return fail(PYCHAIN_HIP_EINVAL, "den_plan_info: a table of the plan lies outside the blob");
    }
    memset(info, 0, 8 * sizeof(int32_t));
    info[0] = gh->H; info[1] = gh->K; info[2] = gh->D;
    info[3] = (int32_t)(gh->total_bytes & 0x7fffffff);   // plan bytes = info[3] + (info[5] << 31): plans beyond 2 GiB keep their exact size
    info[5] = (int32_t)(gh->total_bytes >> 31);
    info[4] = PYCHAIN_HIP_HINT_GENERAL;          // launch hint: the general kernels (den_general.hip)
    return PYCHAIN_HIP_OK;
  }
  const PlanHeader* hd = (const PlanHeader*)host_blob;
  if (hd->magic != PLAN_MAGIC || hd->version != PLAN_VERSION || (size_t)hd->total_bytes > blob_bytes ||
      (size_t)hd->total_bytes < sizeof(PlanHeader))
    return fail(PYCHAIN_HIP_EINVAL, "den_plan_info: not a plan of this library version");
  // the kernels follow the blob's offsets, wave tables and packed LDS addresses unchecked: a blob that comes back from a
  // file (the on-disk plan cache) must be the bytes pychain_hip_den_plan_build wrote
  if ((int32_t)plan_payload_hash(host_blob, (size_t)hd->total_bytes) != hd->payload_hash ||
      (int32_t)plan_header_hash(*hd) != hd->header_hash)
    return fail(PYCHAIN_HIP_EINVAL, "den_plan_info: plan does not match its checksums (corrupted or foreign file)");
  if (!plan_header_in_bounds(*hd))
    return fail(PYCHAIN_HIP_EINVAL, "den_plan_info: a table of the plan lies outside the blob");
  memset(info, 0, 8 * sizeof(int32_t));
  info[0] = hd->H; info[1] = hd->K; info[2] = hd->D; info[3] = hd->total_bytes;
  // the launch hint (plan_format.h: LaunchHint; encode_hint saturates the row counts at their widths)
  LaunchHint lh;
  lh.rows = std::max(hd->alpha.max_wave_slot_rows, hd->beta.max_wave_slot_rows);
  lh.occ_rows = hd->gamma.max_wave_slot_rows;
  lh.occ2_rows = hd->gamma2.max_wave_slot_rows;
  // the plan holds the recursion tiles dealt to FOUR waves (small graphs: den_recursion_lazy_kernel<small>); the
  // recursion field is then the row count of THAT dealing (>= the 16-wave one: a kernel sized by it fits either)
  lh.four_waves = hd->alpha4.nwaves == PLAN_REC4_WAVES && hd->beta4.nwaves == PLAN_REC4_WAVES &&
                  hd->rec4_max_wave_groups >= 1 && hd->rec4_max_wave_groups <= 4;
  if (lh.four_waves) lh.rows = std::max(lh.rows, std::max(hd->alpha4.max_wave_slot_rows, hd->beta4.max_wave_slot_rows));
  // every recursion wave owns at most 4 groups (what den_recursion_lazy_kernel keeps in registers)
  lh.four_groups = hd->rec_max_wave_groups >= 1 && hd->rec_max_wave_groups <= 4;
  // a state sits on several positions of the beta numbering (plan.cpp, "states on several lanes"): not for
  // den_recursion_pair_kernel, whose normalise pass gives every position the constant c(t)
  lh.no_const = hd->n_no_const > 0;
  // every state sits on ONE position of either numbering and every leaky probability is positive (>= 1e-12): the lazy
  // recursions' one-word state vectors (den_lazy.inc.h: MAP::kQ - alpha gathers a / cl, which needs cl > 0 everywhere)
  lh.one_word = hd->n_no_const == 0 && hd->H == hd->graph_states;
  if (lh.one_word) {
    const float* lk = (const float*)((const char*)host_blob + hd->off_leaky_a);
    for (int i = 0; i < hd->H; i++) lh.one_word = lh.one_word && lk[i] >= 1e-12f && lk[i] <= 1e12f;
  }
  // "pdf by state" - every arc entering a state carries one pdf: the lazy recursions' one-gather form (den_lazy.inc.h: SG)
  lh.pdf_by_state = (hd->flags & PLAN_FLAG_PDF_BY_STATE) != 0;
  info[4] = encode_hint(lh);
  info[6] = hd->graph_states;                     // the graph's states (info[0]: positions of the longer side = what calls pass as num_states)
  info[7] = hd->H - hd->graph_states;            // positions added by states on several lanes (the longer side)
  return PYCHAIN_HIP_OK;
}

namespace {
// The denominator workspace: byte offsets of its regions from the 256-aligned base - the size queries and fill_den_args read this.
struct DenCarve { size_t alpha, beta, seq_progress, progress, xprog, tot_a, tot_b, gtot, fin_dot, splice, ex, min_total, total; };
// words of the counter block `progress` (256 bytes; the first kMaxSegments: the gates' counters, DenArgs::progress)
enum { kCtrOccDone = 24 /* a cache line of its own: polled while the queue head is drawn from */, kCtrStreamNext = 32, kCtrFinishCount = 40,
       kCtrRedo = 48, kCtrInvNorm = 56 /* the reciprocal normaliser of the fused loss (chain_loss_forward_one) */ };
DenCarve den_carve(int B, int T, int H, int D) {
  const size_t b = B, Hp = roundup64(H);
  DenCarve c;
  c.alpha = 0;                                                   // [B,T,Hp]
  c.beta = c.alpha + align256(4 * b * T * Hp);                   // [B,T+1,Hp]
  c.seq_progress = c.beta + align256(4 * b * (T + 1) * Hp);      // [2][B]; from here to tot_a: the counters every call zeroes
  c.progress = c.seq_progress + align256(8 * b);
  c.xprog = c.progress + 256;                                    // [2][B][kExMaxQ], then xnan [B]
  c.tot_a = c.xprog + align256(4 * (2 * kExMaxQ + 1) * b);       // per-frame totals of the two recursions, [B,T+2] each
  c.tot_b = c.tot_a + align256(4 * b * (T + 2));
  c.gtot = c.tot_b + align256(4 * b * (T + 2));                  // frame totals to check
  c.fin_dot = c.gtot + align256(4 * b * T);                      // final dot products; den_finish_kernel's per-sequence side of the check
  c.splice = c.fin_dot + align256(8 * b) + 256;                  // time segments: the speculated rows next to the segments (DenArgs::splice)
  c.ex = c.min_total = c.splice + align256(4 * b * 2 * kMaxTimeSegs * 2 * Hp);
  c.total = c.ex + align256(4 * b * T * D);                      // rows exp'd ahead of the recursions (DenArgs::ex): optional
  return c;
}
}  // namespace
extern "C" size_t pychain_hip_den_workspace_min_bytes(int B, int T, int H, int D) {
  return (B <= 0 || T <= 0 || H <= 0 || D <= 0) ? 0 : den_carve(B, T, H, D).min_total;
}
extern "C" size_t pychain_hip_den_workspace_bytes(int B, int T, int H, int D) {
  return (B <= 0 || T <= 0 || H <= 0 || D <= 0) ? 0 : den_carve(B, T, H, D).total;
}

namespace {
int32_t* tstate_of(const void* plans_dev);
// the denominator plan(s) of a call: the device blob, the bytes from one sequence's plan to the next (0: one for all), the launch
// hint and the positions pychain_hip_den_plan_info reports
struct DenPlan { const void* blob; int64_t stride_bytes; int hint, H; };
int fill_den_args(DenArgs& a, const DenPlan& plan, const Rows& rows, int input_is_exp, float leaky_hmm_coefficient, float grad_scale,
                  float* objf_per_seq, void* grad, int32_t* bad_count, const Workspace& wsp, const char* who) {
  const int H = plan.H, B = rows.B, T = rows.T, D = rows.D;
  if (int rc = bad_dtype(who, rows.dtype)) return rc;
  if (!plan.blob || !rows.x || !rows.lengths || !objf_per_seq || !grad || !bad_count || !wsp.p) return null_pointer(who);
  if (B <= 0 || T <= 0 || H <= 0 || D <= 0)
    return fail(PYCHAIN_HIP_EINVAL, "%s: bad sizes B=%d T=%d H=%d D=%d", who, B, T, H, D);
  if ((H > 65535 || D > 65535) && plan.hint != PYCHAIN_HIP_HINT_GENERAL)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: more than 65535 states or pdfs need a plan in the general format (build it with "
                "pychain_hip_den_plan_build and pass the launch hint pychain_hip_den_plan_info reports)", who);
  // chain-computation.cc:68 asserts 0 < coefficient < 1 (compiled out under NDEBUG); here it is an error
  if (!(leaky_hmm_coefficient > 0.f && leaky_hmm_coefficient < 1.f))
    return fail(PYCHAIN_HIP_EINVAL, "%s: leaky_hmm_coefficient must be in (0,1), got %g", who, (double)leaky_hmm_coefficient);
  if (plan.stride_bytes < 0 || (plan.stride_bytes & 15))
    return fail(PYCHAIN_HIP_EINVAL, "%s: plan stride must be a non-negative multiple of 16", who);
  if (((uintptr_t)plan.blob | (uintptr_t)rows.x | (uintptr_t)grad | (uintptr_t)wsp.p) & 15)
    return fail(PYCHAIN_HIP_EINVAL, "%s: plan, nnet_output, grad and workspace must be 16-byte aligned", who);
  const DenCarve c = den_carve(B, T, H, D);
  if (wsp.bytes < c.min_total)
    return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace too small (%zu < %zu)", who, wsp.bytes, c.min_total);
  den_shape_args(a, plan.stride_bytes, H, D, B, T);      // (zeroes `a`: what is not set below is 0 / null)
  a.plans = (const char*)plan.blob;
  a.x = (const float*)rows.x; a.x_half = rows.dtype; a.lengths = rows.lengths; a.objf = objf_per_seq; a.grad = (float*)grad; a.bad = bad_count;
  a.input_is_exp = input_is_exp ? 1 : 0;
  a.phase_mask = a.knobs.den_phase_mask;
  a.coef = leaky_hmm_coefficient; a.grad_scale = grad_scale;
  a.loss_scale = 1.f; a.bad_words = 1;
  char* ws = ws_base(wsp.p);
  a.alpha_store = (float*)(ws + c.alpha); a.beta_store = (float*)(ws + c.beta);
  a.seq_progress = (int32_t*)(ws + c.seq_progress);
  a.progress = (int32_t*)(ws + c.progress);
  a.occ_done = a.progress + kCtrOccDone; a.stream_next = a.progress + kCtrStreamNext;
  a.finish_count = a.progress + kCtrFinishCount; a.redo = a.progress + kCtrRedo;
  a.xprog = (int32_t*)(ws + c.xprog); a.xnan = a.xprog + 2 * (size_t)B * kExMaxQ;
  a.tot_a = (float*)(ws + c.tot_a); a.tot_b = (float*)(ws + c.tot_b); a.gtot = (float*)(ws + c.gtot); a.fin_dot = (float*)(ws + c.fin_dot);
  a.splice = (float*)(ws + c.splice);
  // (behind everything else, and only in a workspace of the full size: DenArgs::ex)
  a.ex = wsp.bytes >= c.total ? (float*)(ws + c.ex) : nullptr;
  // (the plan's burn-in controller, unless the caller pins the cut or the burn-in with an option of its own)
  a.tstate = (option_set("den_tseg") || option_set("den_tburn")) ? nullptr : tstate_of(plan.blob);
  return PYCHAIN_HIP_OK;
}
}  // namespace

namespace {
// the numerator's tile recursions stage 2-byte rows in their float4-chunk forms (num_fb_kernel); the general and the
// reference-arithmetic kernels read fp32
bool num_half_native(const NumArgs& a) {
  return !a.general && !a.compat && a.D % 4 == 0 && a.D <= 4 * 8 * 512;
}

// Every word a call's launches count in - the caller's bad count(s) and the workspace's counters (per-sequence progress, gate
// counters, the queue head of the streamed occupancy pass, den_finish_kernel's arrival counter) - zeroed by ONE small launch
// (two hipMemsetAsync are two fill kernels with a gap between them: 18 us at the head of every step).
// (`norm` / `inv_out`: the fused loss with a device-side normaliser - *inv_out = 1 / *norm for the occupancy launches of the
// call, which scale the gradient by it; inv_out lies inside p1's range and is written behind its zeroing)
__global__ void zero_words_kernel(int32_t* p0, int n0, int32_t* p1, int n1, const float* norm, float* inv_out) {
  for (int i = threadIdx.x; i < n0; i += blockDim.x) p0[i] = 0;
  for (int i = threadIdx.x; i < n1; i += blockDim.x) p1[i] = 0;
  if (inv_out) {
    __syncthreads();
    if (threadIdx.x == 0) *inv_out = 1.0f / *norm;
  }
}
hipError_t launch_zero_words(int32_t* p0, int n0, int32_t* p1, int n1, hipStream_t st, const float* norm = nullptr, float* inv_out = nullptr) {
  hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(256), 0, st, p0, n0, p1, n1, norm, inv_out);
  return hipGetLastError();
}
// (DenCarve: seq_progress up to tot_a)
int den_counter_words(const DenArgs& a) { return (int)(((const char*)a.tot_a - (const char*)a.seq_progress) / 4); }

}  // namespace

// ---- the burn-in controller state of a plan (DenArgs::tstate): a caller-owned device blob, attached by plan address
namespace {
std::mutex g_tstate_lock;
std::map<const void*, void*>& tstate_table() { static std::map<const void*, void*> t; return t; }
int32_t* tstate_of(const void* plans_dev) {
  std::lock_guard<std::mutex> guard(g_tstate_lock);
  auto it = tstate_table().find(plans_dev);
  return it == tstate_table().end() ? nullptr : (int32_t*)it->second;
}
}  // namespace
extern "C" int pychain_hip_den_tseg_state(const void* plans_dev, void* state_dev) {
  if (!plans_dev) return fail(PYCHAIN_HIP_EINVAL, "den_tseg_state: null plan");
  if (state_dev && ((uintptr_t)state_dev & 3)) return fail(PYCHAIN_HIP_EINVAL, "den_tseg_state: the state must be 4-byte aligned");
  std::lock_guard<std::mutex> guard(g_tstate_lock);
  if (state_dev) tstate_table()[plans_dev] = state_dev; else tstate_table().erase(plans_dev);
  return PYCHAIN_HIP_OK;
}
extern "C" size_t pychain_hip_den_tseg_state_bytes(void) { return kTsegStateWords * sizeof(int32_t); }

extern "C" int pychain_hip_den_uses_row_buffer(int64_t plan_stride_bytes, int hint, int H, int D, int B, int T,
                                              int input_is_exp) {
  if (B <= 0 || T <= 0 || H <= 0 || D <= 0 || hint == PYCHAIN_HIP_HINT_GENERAL) return 0;
  return den_would_exp_rows_ahead(den_query_args(plan_stride_bytes, hint, H, D, B, T, false, input_is_exp != 0)) ? 1 : 0;
}

extern "C" int pychain_hip_den_time_segments(int64_t plan_stride_bytes, int hint, int H, int D, int B, int T, int fused) {
  if (B <= 0 || T <= 0 || H <= 0 || D <= 0 || hint == PYCHAIN_HIP_HINT_GENERAL) return 1;
  return den_time_segments(den_query_args(plan_stride_bytes, hint, H, D, B, T, fused != 0), fused != 0);
}
namespace {
int den_half_native_q(int64_t plan_stride_bytes, int hint, int H, int D, int B, int T, bool fused) {
  if (B <= 0 || T <= 0 || H <= 0 || D <= 0) return 0;
  return den_call_half_native(den_query_args(plan_stride_bytes, hint, H, D, B, T, fused), hint) ? 1 : 0;
}
}  // namespace
extern "C" int pychain_hip_den_half_native(int64_t plan_stride_bytes, int hint, int H, int D, int B, int T) {
  return den_half_native_q(plan_stride_bytes, hint, H, D, B, T, false);
}
extern "C" int pychain_hip_num_half_native(int H, int K, int D) {
  if (H <= 0 || K <= 0 || D <= 0) return 0;
  NumArgs n;
  memset(&n, 0, sizeof(n));
  n.H = H; n.K = K; n.D = D; n.general = num_needs_general(H, K, D) ? 1 : 0; n.compat = call_knobs().num_compat;
  return num_half_native(n) ? 1 : 0;
}
extern "C" int pychain_hip_chain_loss_half_native(int64_t plan_stride_bytes, int hint, int den_H, int D, int B, int T,
                                                  int num_H, int num_K) {
  if (!den_half_native_q(plan_stride_bytes, hint, den_H, D, B, T, true) || !pychain_hip_num_half_native(num_H, num_K, D)) return 0;
  DenArgs a = den_query_args(plan_stride_bytes, hint, den_H, D, B, T, true);
  a.fold_rows = (const float*)1;                          // (the fold's extra LDS counts: gamma2_lds_bytes)
  return den_uses_gamma2(a, (D + 63) / 64, hint) ? 1 : 0;
}

// ---- test hook: a long-lived kernel that pins CUs on another stream of the same process, as the channels of an overlapped
// RCCL bucket all-reduce do during DDP's backward: `workgroups` workgroups of 1024 threads and 100 KB of LDS
// (one to a CU), each sleeping for `microseconds`
namespace {
__global__ __launch_bounds__(1024) void occupy_kernel(unsigned long long ticks, int* sink) {
  extern __shared__ char occ_lds[];
  const unsigned long long t0 = wall_clock64();                   // 100 MHz
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
  if (sink && threadIdx.x == 0 && occ_lds[threadIdx.x] == 77) *sink = 1;
}
}  // namespace
extern "C" int pychain_hip_debug_occupy(int workgroups, int microseconds, void* stream) {
  if (workgroups <= 0 || microseconds < 0 || microseconds > 2000000) return fail(PYCHAIN_HIP_EINVAL, "debug_occupy: bad arguments");
  const int lds = 100 * 1024;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(occupy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return fail(PYCHAIN_HIP_ELAUNCH, "debug_occupy: cannot set the LDS size");
  hipLaunchKernelGGL(occupy_kernel, dim3(workgroups), dim3(1024), lds, (hipStream_t)stream, (unsigned long long)microseconds * 100ull, (int*)nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "debug_occupy: %s", hipGetErrorString(e));
  return PYCHAIN_HIP_OK;
}

extern "C" int pychain_hip_debug_stream_rings(int T, int32_t* out, int out_len, int32_t* report_due, int due_len) {
  if (T <= 0 || out_len < 0 || due_len < 0 || (out_len && !out) || (due_len && !report_due))
    return fail(PYCHAIN_HIP_EINVAL, "debug_stream_rings: bad arguments");
  const int n = stream_ring_count(T);
  for (int r = 0; r < n && 2 * r + 1 < out_len; r++) {
    int lo, hi;
    stream_ring(T, r, lo, hi);
    out[2 * r] = lo; out[2 * r + 1] = hi;
  }
  for (int d = 0; d < due_len; d++) report_due[d] = stream_report_due(T, d) ? 1 : 0;
  return n;
}

extern "C" int pychain_hip_debug_launch_map(int T, int L, int t, int frames_per_block, int nseg,
                                            const int32_t* seg_bound, int seg, int32_t* out, int out_len) {
  if (T <= 0 || L <= 0 || L > T || frames_per_block <= 0 || nseg < 0 || nseg > 16 || (nseg && !seg_bound) || seg < 0 || (nseg && seg >= nseg))
    return fail(PYCHAIN_HIP_EINVAL, "debug_launch_map: bad arguments");
  return den_debug_launch_map(T, L, t, frames_per_block, nseg, seg_bound, seg, out, out_len);
}

extern "C" int pychain_hip_den_forward_backward(
    const void* plans_dev, int64_t plan_stride_bytes, int hint, int H, int D,
    const void* nnet_output, int nnet_output_dtype, int input_is_exp, const int64_t* seq_lengths,
    int B, int T, float leaky_hmm_coefficient, float grad_scale,
    float* objf_per_seq, void* grad, int32_t* bad_count, float* totals,
    void* workspace, size_t workspace_bytes, void* stream) {
  DenArgs a;
  if (int rc = fill_den_args(a, DenPlan{plans_dev, plan_stride_bytes, hint, H}, Rows{nnet_output, nnet_output_dtype, seq_lengths, B, T, D},
                             input_is_exp, leaky_hmm_coefficient, grad_scale, objf_per_seq, grad, bad_count,
                             Workspace{workspace, workspace_bytes}, "den_forward_backward")) return rc;
  a.loss_out = totals;                                 // (sum of the per-sequence objectives, frames, bad count: den_finish_kernel)
  if (a.x_half && !den_call_half_native(a, hint))
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "den_forward_backward: this shape does not take 2-byte network outputs (pychain_hip_den_half_native)");
  hipStream_t st = (hipStream_t)stream;
  if (launch_zero_words(bad_count, 1, a.seq_progress, den_counter_words(a), st) != hipSuccess)
    return fail(PYCHAIN_HIP_ELAUNCH, "den_forward_backward: cannot zero the counters");
  const char* why = nullptr;
  hipError_t e = run_den(a, hint, true, st, &why);
  return e == hipSuccess ? PYCHAIN_HIP_OK : launch_failed("den_forward_backward", e, why);
}

namespace {
struct NumCarve { size_t alpha, beta, logp, rows, upd, ucount, uidx, frac, gacc, compat, total; };
NumCarve num_carve(int B, int T, int H, int K, int D, bool compat) {
  NumCarve c;
  c.alpha = 0;
  c.beta = c.alpha + align256(8 * (size_t)B * (T + 1) * H);
  c.logp = c.beta + align256(8 * (size_t)B * (T + 1) * H);
  c.rows = c.logp + align256(8 * (size_t)B);
  c.upd = c.rows + align256(4 * (size_t)B * T * K);
  c.ucount = c.upd + align256(4 * (size_t)B * K);
  c.uidx = c.ucount + align256(4 * (size_t)B);
  c.frac = c.uidx + align256(4 * (size_t)B * K);
  c.gacc = c.frac + align256(4 * (size_t)B * T * K);           // general kernels only (num_general.hip): accumulator rows
  c.compat = c.gacc + (num_needs_general(H, K, D) ? align256(num_general_acc_bytes(D)) : 0);
  c.total = c.compat + (compat ? (size_t)B * num_compat_stride(H, K) : 0) + 256;   // (option num_compat: num_compat.hip)
  return c;
}

int fill_num_args(NumArgs& a, const NumGraphs& g, const Rows& rows, int grad_mode, float grad_scale,
                  float* objf_per_seq, void* grad, int32_t* bad_count, const Workspace& wsp, const char* who, const int32_t* windows) {
  const int B = rows.B, T = rows.T, D = rows.D, H = g.H, K = g.K;
  if (int rc = bad_dtype(who, rows.dtype)) return rc;
  if (g.any_null() || !rows.x || !rows.lengths || !objf_per_seq || !grad || !bad_count || !wsp.p) return null_pointer(who);
  if (int rc = bad_sizes(who, rows, g)) return rc;
  if (int rc = bad_stride(who, g.stride)) return rc;
  if (grad_mode < PYCHAIN_HIP_GRAD_LOG || grad_mode > PYCHAIN_HIP_GRAD_ACCUM)
    return fail(PYCHAIN_HIP_EINVAL, "%s: unknown grad_mode %d", who, grad_mode);
  if (((uintptr_t)rows.x | (uintptr_t)grad | (uintptr_t)g.fi | (uintptr_t)g.bi) & 15)
    return fail(PYCHAIN_HIP_EINVAL, "%s: nnet_output, grad and index tensors must be 16-byte aligned", who);
  const CallKnobs knobs = call_knobs();
  const NumCarve c = num_carve(B, T, H, K, D, knobs.num_compat != 0);
  if (wsp.bytes < c.total) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace too small", who);
  if (windows && knobs.num_compat)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: option num_compat (the reference's own arithmetic) takes no alignment time windows", who);
  memset(&a, 0, sizeof(a));
  a.fwd_trans = g.ft; a.fwd_idx = g.fi; a.fwd_probs = g.fp; a.bwd_trans = g.bt; a.bwd_idx = g.bi; a.bwd_probs = g.bp;
  a.initial = g.initial; a.final_ = g.final_; a.x = (const float*)rows.x; a.x_half = rows.dtype; a.lengths = rows.lengths;
  a.objf = objf_per_seq; a.grad = (float*)grad; a.bad = bad_count;
  a.graph_stride = g.stride; a.B = B; a.T = T; a.D = D; a.H = H; a.K = K;
  a.grad_mode = grad_mode; a.grad_scale = grad_scale; a.frames_per_block = 32;
  a.check_all = knobs.verbose >= 1 ? 1 : 0;
  if (knobs.corrupt_what == 2 && knobs.corrupt_b < B && knobs.corrupt_t < T) {
    a.corrupt_b = knobs.corrupt_b; a.corrupt_t = knobs.corrupt_t; a.corrupt_log = logf(knobs.corrupt_scale);
  } else a.corrupt_b = -1;
  a.watch_nan = 1;                                   // (the fused loss clears it: NumArgs::watch_nan)
  char* ws = ws_base(wsp.p);
  a.alpha_ws = (double*)(ws + c.alpha); a.beta_ws = (double*)(ws + c.beta); a.logp_ws = (double*)(ws + c.logp);
  a.rows_ws = (float*)(ws + c.rows); a.upd_ws = (int32_t*)(ws + c.upd); a.ucount_ws = (int32_t*)(ws + c.ucount);
  a.uidx_ws = (int32_t*)(ws + c.uidx); a.frac_ws = (float*)(ws + c.frac);
  a.general = num_needs_general(H, K, D) ? 1 : 0;             // graphs beyond the tile kernels: num_general.hip
  a.gen_acc = ws + c.gacc;
  a.compat = knobs.num_compat; a.compat_ws = ws + c.compat; a.compat_stride = num_compat_stride(H, K);
  a.windows = windows;                                       // (NumArgs::windows; nullptr = none)
  return PYCHAIN_HIP_OK;
}
}  // namespace


// ---- numerator posteriors as cross-entropy targets (include/pychain_hip.h: pychain_hip_xent; xent.hip) ------------------
namespace {
// a checked pychain_hip_xent with the pointers of the sequences ONE call (or one slice of a call) is given
struct XentCall {
  const char* z; int z_dtype; char* grad; float grad_scale; const float* grad_scale_dev; float* objf;
  double* frame_objf;        // [B,T] frame objectives (workspace)
  float* dense;              // [B,T,D] dense posteriors: numerator graphs on the general kernels only (workspace)
  int32_t* scratch_bad;      // where an occupancy launch made for xent alone counts (the caller's bad count stays as it was)
};
struct XentCarve { size_t scratch, frames, dense, total; };
XentCarve xent_carve(int B, int T, int H, int K, int D) {
  XentCarve c;
  c.scratch = 0;
  c.frames = 256;
  c.dense = c.frames + align256(xent_frame_bytes(B, T));
  c.total = c.dense + (num_needs_general(H, K, D) ? align256(4 * (size_t)B * T * D) : 0) + 256;
  return c;
}
int xent_check(const pychain_hip_xent* x, int B, int T, int H, int K, int D, const char* who, XentCall& out) {
  if (int rc = bad_sizes(who, B, T, H, K, D)) return rc;
  if (!x->z || !x->xent_objf_per_seq || !x->workspace) return fail(PYCHAIN_HIP_EINVAL, "%s: xent: null z, xent_objf_per_seq or workspace", who);
  if (x->z_dtype < PYCHAIN_HIP_F32 || x->z_dtype > PYCHAIN_HIP_F16) return fail(PYCHAIN_HIP_EINVAL, "%s: xent: unknown z_dtype %d", who, x->z_dtype);
  if (((uintptr_t)x->z | (uintptr_t)x->xent_grad | (uintptr_t)x->workspace) & 15)
    return fail(PYCHAIN_HIP_EINVAL, "%s: xent: z, xent_grad and workspace must be 16-byte aligned", who);
  if (call_knobs().num_compat)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: option num_compat (the reference's own arithmetic) takes no cross-entropy output", who);
  const XentCarve c = xent_carve(B, T, H, K, D);
  if (x->workspace_bytes < c.total) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: xent workspace too small (%zu < %zu)", who, x->workspace_bytes, c.total);
  char* ws = ws_base(x->workspace);
  out.z = (const char*)x->z; out.z_dtype = x->z_dtype; out.grad = (char*)x->xent_grad;
  out.grad_scale = x->grad_scale; out.grad_scale_dev = x->grad_scale_dev; out.objf = x->xent_objf_per_seq;
  out.scratch_bad = (int32_t*)(ws + c.scratch);
  out.frame_objf = (double*)(ws + c.frames);
  out.dense = num_needs_general(H, K, D) ? (float*)(ws + c.dense) : nullptr;
  return PYCHAIN_HIP_OK;
}
// the same call over the sequences from b0 on (a slice: the workspace is reused, slice after slice in stream order)
XentCall xent_slice(const XentCall& x, int b0, int T, int D) {
  XentCall s = x;
  const size_t off = Rows{x.z, x.z_dtype, nullptr, 0, T, D}.offset(b0);
  s.z = x.z + off;
  if (x.grad) s.grad = x.grad + off;
  s.objf = x.objf + b0;
  return s;
}
// the row kernel over the occupancies `na`'s launches left: the compact rows of the tile path, or (general kernels) a dense
// posterior buffer an occupancy launch of its own fills first - everything on `st`, behind the recursions
hipError_t run_xent(const NumArgs& na, const XentCall& xc, const float* norm_dev, hipStream_t st, const char** why) {
  XentArgs xa;
  memset(&xa, 0, sizeof(xa));
  xa.z = xc.z; xa.z_half = xc.z_dtype; xa.grad = xc.grad; xa.scale = xc.grad_scale; xa.scale_dev = xc.grad_scale_dev; xa.norm_dev = norm_dev;
  xa.lengths = na.lengths; xa.logp = na.logp_ws; xa.frame_objf = xc.frame_objf; xa.objf = xc.objf;
  xa.B = na.B; xa.T = na.T; xa.D = na.D;
  if (na.general) {
    NumArgs d = na;
    d.grad = xc.dense; d.grad_mode = PYCHAIN_HIP_GRAD_LINEAR; d.grad_scale = 1.f; d.grad_scale_dev = nullptr; d.bad = xc.scratch_bad;
    hipError_t e = launch_num_occ(d, false, st, why);
    if (e != hipSuccess) return e;
    xa.dense = xc.dense;
  } else {
    xa.rows = na.rows_ws; xa.upd = na.upd_ws; xa.ucount = na.ucount_ws; xa.K = na.K;
  }
  return launch_xent_rows(xa, st, why);
}
}  // namespace

extern "C" size_t pychain_hip_xent_workspace_bytes(int B, int T, int H, int K, int D) {
  if (B <= 0 || T <= 0 || H <= 0 || K <= 0 || D <= 0) return 0;
  return xent_carve(B, T, H, K, D).total;
}

extern "C" size_t pychain_hip_num_workspace_bytes(int B, int T, int H, int K, int D) {
  if (B <= 0 || T <= 0 || H <= 0 || K <= 0 || D <= 0) return 0;
  return num_carve(B, T, H, K, D, call_knobs().num_compat != 0).total;   // (the calling thread's options, as the call will read them)
}

extern "C" int pychain_hip_num_forward_backward_xent(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int D, int H, int K, int grad_mode, float grad_scale, float* objf_per_seq, float* grad, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream, const int32_t* time_windows, const pychain_hip_xent* xent) {
  NumArgs a;
  XentCall xc;
  if (xent) { if (int rc = xent_check(xent, B, T, H, K, D, "num_forward_backward", xc)) return rc; }
  const bool dense_grad = grad != nullptr || !xent;      // (with xent `grad` may be NULL: only the cross-entropy is wanted)
  if (int rc = fill_num_args(a, NumGraphs{ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, H, K},
                             Rows{nnet_output, nnet_output_dtype, seq_lengths, B, T, D}, grad_mode, grad_scale, objf_per_seq,
                             dense_grad ? (void*)grad : workspace, bad_count, Workspace{workspace, workspace_bytes}, "num_forward_backward",
                             time_windows)) return rc;
  // (2-byte network outputs are READ as they are by the tile recursions; the gradient of this entry point stays fp32)
  if (a.x_half && !num_half_native(a))
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "num_forward_backward: this shape does not take 2-byte network outputs (pychain_hip_num_half_native)");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(bad_count, 0, sizeof(int32_t), st) != hipSuccess)
    return fail(PYCHAIN_HIP_ELAUNCH, "num_forward_backward: hipMemsetAsync failed");
  const char* why = nullptr;
  hipError_t e = hipSuccess;
  if (a.compat) {                                        // the reference's own arithmetic, one launch (num_compat.hip)
    e = launch_num_compat(a, 3, st);
  } else {
    e = launch_num_fb(a, st, &why);
    if (e == hipSuccess && a.corrupt_b >= 0) e = launch_num_corrupt(a, st);
    if (e == hipSuccess && dense_grad) e = launch_num_occ(a, false, st, &why);
    if (e == hipSuccess && xent) {
      // the compact rows of the tile path for the row kernel (their own checks count into a scratch word: bad_count is the
      // call's without xent), then the rows and the sums
      NumArgs c = a;
      c.bad = xc.scratch_bad;
      if (!a.general) {
        e = launch_num_prep(c, st, &why);
        if (e == hipSuccess) e = launch_num_occ(c, true, st, &why);
      }
      if (e == hipSuccess) e = run_xent(a, xc, nullptr, st, &why);
      if (e == hipSuccess && xent->xent_totals) e = launch_xent_totals(xc.objf, B, 1.f, nullptr, 0.f, xent->xent_totals, nullptr, st);
    }
  }
  return e == hipSuccess ? PYCHAIN_HIP_OK : launch_failed("num_forward_backward", e, why);
}

extern "C" int pychain_hip_num_forward_backward_tw(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int D, int H, int K, int grad_mode, float grad_scale, float* objf_per_seq, float* grad, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream, const int32_t* time_windows) {
  return pychain_hip_num_forward_backward_xent(ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, nnet_output, nnet_output_dtype,
                                               seq_lengths, B, T, D, H, K, grad_mode, grad_scale, objf_per_seq, grad, bad_count,
                                               workspace, workspace_bytes, stream, time_windows, nullptr);
}

extern "C" int pychain_hip_num_forward_backward(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int D, int H, int K, int grad_mode, float grad_scale, float* objf_per_seq, float* grad, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream) {
  return pychain_hip_num_forward_backward_tw(ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, nnet_output, nnet_output_dtype,
                                             seq_lengths, B, T, D, H, K, grad_mode, grad_scale, objf_per_seq, grad, bad_count,
                                             workspace, workspace_bytes, stream, nullptr);
}

// ---- expected arc counts of the numerator (include/pychain_hip.h: pychain_hip_num_arc_counts; num_arcs.hip)
namespace {
// the numerator's workspace (num_carve), then: the float objective the recursion writes, lp + w in both arc orders, a copy per
// sequence of a shared graph's other arrays (used only by a call with weights on a shared graph; always carved: the size query
// does not know the stride), the partial rows
struct NumArcCarve { size_t objf, wf, wb, rft, rbt, rfi, rbi, rinit, rfin, partial, total; int nrun; };
NumArcCarve num_arc_carve(int B, int T, int H, int K, int D, bool compat) {
  NumArcCarve c;
  const size_t b = B, probs = align256(4 * b * K), trans = align256(12 * b * K), idx = align256(8 * b * H), vec = align256(4 * b * H);
  c.nrun = (T + kNumArcFrames - 1) / kNumArcFrames;
  size_t o = align256(num_carve(B, T, H, K, D, compat).total);
  c.objf = o; o += align256(4 * b);
  c.wf = o; o += probs; c.wb = o; o += probs;
  c.rft = o; o += trans; c.rbt = o; o += trans;
  c.rfi = o; o += idx; c.rbi = o; o += idx;
  c.rinit = o; o += vec; c.rfin = o; o += vec;
  c.partial = o; o += align256(8 * b * c.nrun * K);
  c.total = o + 256;                                 // (the base is aligned inside the caller's buffer)
  return c;
}
}  // namespace

extern "C" size_t pychain_hip_num_arc_counts_workspace_bytes(int B, int T, int H, int K, int D) {
  if (B <= 0 || T <= 0 || H <= 0 || K <= 0 || D <= 0) return 0;
  return num_arc_carve(B, T, H, K, D, false).total;
}

extern "C" int pychain_hip_num_arc_counts(
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int D, int H, int K, int grad_mode, float grad_scale, const float* arc_log_weights,
    double* objf_per_seq, float* grad, double* counts_per_seq, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream, const int32_t* time_windows) {
  const char* who = "num_arc_counts";
  if (!counts_per_seq || !objf_per_seq) return null_pointer(who);
  if (int rc = bad_sizes(who, B, T, H, K, D)) return rc;
  if (grad_mode != PYCHAIN_HIP_GRAD_LINEAR && grad_mode != PYCHAIN_HIP_GRAD_ACCUM)
    return fail(PYCHAIN_HIP_EINVAL, "%s: grad_mode must be PYCHAIN_HIP_GRAD_LINEAR or PYCHAIN_HIP_GRAD_ACCUM, got %d (the log form is "
                "the reference's contract for its own gradient, not a gradient beside arc counts)", who, grad_mode);
  const CallKnobs knobs = call_knobs();
  if (knobs.num_compat)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: option num_compat (the reference's own arithmetic) takes no arc weights and leaves no "
                "arc log-shares to count from", who);
  const NumArcCarve c = num_arc_carve(B, T, H, K, D, false);
  if (!workspace) return null_pointer(who);
  if (workspace_bytes < c.total) return fail(PYCHAIN_HIP_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, c.total);
  char* ws = ws_base(workspace);
  NumArgs a;
  if (int rc = fill_num_args(a, NumGraphs{ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, H, K},
                             Rows{nnet_output, nnet_output_dtype, seq_lengths, B, T, D}, grad_mode, grad_scale, (float*)(ws + c.objf),
                             grad ? (void*)grad : (void*)ws, bad_count, Workspace{workspace, workspace_bytes}, who, time_windows)) return rc;
  if (a.x_half && !num_half_native(a))
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: this shape does not take 2-byte network outputs (pychain_hip_num_half_native)", who);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(bad_count, 0, 2 * sizeof(int32_t), st) != hipSuccess)
    return fail(PYCHAIN_HIP_ELAUNCH, "%s: hipMemsetAsync failed", who);
  const char* why = nullptr;
  hipError_t e = hipSuccess;
  if (arc_log_weights) {
    // the weighted graph: two substituted probability buffers [B,K] - and, for a shared graph, a copy per sequence of the
    // arrays they are indexed with, so that the recursion kernels run as they are (one stride for all of a graph's arrays)
    NumArcWeightArgs w;
    memset(&w, 0, sizeof(w));
    w.ft = ft; w.fi = fi; w.fp = fp; w.bt = bt; w.bi = bi; w.bp = bp; w.initial = initial; w.final_ = final_;
    w.graph_stride = graph_batch_stride; w.B = B; w.H = H; w.K = K; w.w = arc_log_weights;
    w.wf = (float*)(ws + c.wf); w.wb = (float*)(ws + c.wb); w.bad = bad_count + 1;
    if (graph_batch_stride == 0) {
      w.rft = (int32_t*)(ws + c.rft); w.rbt = (int32_t*)(ws + c.rbt); w.rfi = (int32_t*)(ws + c.rfi); w.rbi = (int32_t*)(ws + c.rbi);
      w.rinit = (float*)(ws + c.rinit); w.rfin = (float*)(ws + c.rfin);
      a.fwd_trans = w.rft; a.bwd_trans = w.rbt; a.fwd_idx = w.rfi; a.bwd_idx = w.rbi; a.initial = w.rinit; a.final_ = w.rfin;
      a.graph_stride = 1;
    }
    a.fwd_probs = w.wf; a.bwd_probs = w.wb;
    e = launch_num_arc_weights(w, st);
  }
  if (e == hipSuccess) e = launch_num_fb(a, st, &why);
  if (e == hipSuccess && a.corrupt_b >= 0) e = launch_num_corrupt(a, st);
  if (e == hipSuccess && grad) e = launch_num_occ(a, false, st, &why);
  if (e == hipSuccess) {
    NumArcArgs ca;
    ca.n = a; ca.partial = (double*)(ws + c.partial); ca.counts = counts_per_seq; ca.objf = objf_per_seq; ca.nrun = c.nrun;
    e = launch_num_arc_counts(ca, knobs.num_arcs_gather != 0, st);
  }
  return e == hipSuccess ? PYCHAIN_HIP_OK : launch_failed(who, e, why);
}

// ---- fused ChainLoss ------------------------------------------------------------------

namespace {
// the arguments of pychain_hip_chain_loss_forward_xent (include/pychain_hip.h), packed once: of the whole call, or of one slice
struct ChainLossCall {
  DenPlan plan; float leaky;
  NumGraphs graphs; Rows rows;
  float* den_objf; float* num_objf; void* grad; float grad_scale; int32_t* bad_count;      // [B], [B], [B,T,D] as the rows or null, [2]
  float loss_scale; const float* loss_norm_dev; float* totals;
  Workspace den_ws, num_ws; hipStream_t stream; const int32_t* windows;
  const XentCall* xent;                                                                    // checked (xent_check), or null
};
// one fused call over the B sequences it is given (pychain_hip_chain_loss_forward: all of them, or one slice of a large batch)
int chain_loss_forward_one(const ChainLossCall& c) {
  const char* who = "chain_loss_forward";
  void* const grad = c.grad; const float* const loss_norm_dev = c.loss_norm_dev; const XentCall* const xc = c.xent;
  const int hint = c.plan.hint;
  if (!c.bad_count) return fail(PYCHAIN_HIP_EINVAL, "%s: null bad_count", who);
  DenArgs da;
  // without `grad` only the recursions run; any non-null aligned pointer then passes the checks
  if (int rc = fill_den_args(da, c.plan, c.rows, 0, c.leaky, c.grad_scale, c.den_objf, grad ? grad : c.den_ws.p, c.bad_count, c.den_ws, who)) return rc;
  NumArgs na;
  if (int rc = fill_num_args(na, c.graphs, c.rows, PYCHAIN_HIP_GRAD_ACCUM, -c.grad_scale, c.num_objf, grad ? grad : c.num_ws.p, c.bad_count + 1,
                             c.num_ws, who, c.windows)) return rc;

  da.fused = 1;
  na.watch_nan = 0;              // the denominator's alpha workgroups watch every element of every row (NumArgs::watch_nan)
  // the scalars of ChainLoss.forward from den_finish_kernel's last workgroup (DenArgs::loss_out)
  da.loss_out = c.totals; da.loss_num_objf = c.num_objf; da.loss_scale = c.loss_scale; da.loss_norm_dev = loss_norm_dev; da.bad_words = 2;
  hipStream_t st = c.stream;
  SideStream* side = side_streams_for(st);
  if (!side) return fail(PYCHAIN_HIP_ELAUNCH, "%s: cannot create the side stream", who);
  const char* why = nullptr;
  // a device-side normaliser of the loss (loss_norm_dev: ChainLoss(avg=True) with the lengths on the device) also divides the
  // gradient written here: its reciprocal goes into a spare counter word at the head of the call and the occupancy launches
  // of both sides read it (DenArgs / NumArgs::grad_scale_dev) - not a pass over [B, T, D] behind the call
  float* inv_norm = (loss_norm_dev && grad) ? reinterpret_cast<float*>(da.progress + kCtrInvNorm) : nullptr;
  if (inv_norm) { da.grad_scale_dev = inv_norm; na.grad_scale_dev = inv_norm; }
  hipError_t e = launch_zero_words(c.bad_count, 2, da.seq_progress, den_counter_words(da), st, loss_norm_dev, inv_norm);
  // The two-frame occupancy kernel folds the numerator in (grad = scale * (gamma_den - gamma_num), written
  // once): the numerator then also produces compact occupancy rows on its stream, and the occupancy
  // launches wait for them.  Otherwise the numerator is accumulated into the gradient afterwards.
  // (decided with the fold's own LDS rows counted in: gamma2_lds_bytes)
  da.fold_rows = na.rows_ws;
  const bool fold = grad && hint != PYCHAIN_HIP_HINT_GENERAL && !na.general && !na.compat &&
                    den_uses_gamma2(da, (c.rows.D + 63) / 64, hint);
  if (fold) {
    da.fold_upd = na.upd_ws; da.fold_ucount = na.ucount_ws; da.fold_K = c.graphs.K;
    da.fold_scale = -c.grad_scale;
  } else da.fold_rows = nullptr;
  // 2-byte network outputs: both sides take them and the gradient is written once, by the fold (chain_loss_half_native)
  if (c.rows.dtype != PYCHAIN_HIP_F32 && !(den_call_half_native(da, hint) && num_half_native(na) && (fold || !grad)))
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: this shape does not take 2-byte network outputs (pychain_hip_chain_loss_half_native)", who);
  // fork: numerator on the side stream, denominator recursion on the caller's stream
  if (e == hipSuccess) e = hipEventRecord(side->fork, st);
  if (e == hipSuccess) e = hipStreamWaitEvent(side->stream, side->fork, 0);
  // (option num_compat: the numerator is ONE launch behind the denominator's occupancy launches - it accumulates into the
  // gradient they wrote - and in front of den_finish_kernel, which reads its log-probabilities)
  // (xent on the tile path reads the compact rows: a call without `grad` then produces them too - into the same workspace, its
  // checks counted into a scratch word, so that bad_count is the call's without xent)
  const bool xcompact = xc && !na.general;
  if (e == hipSuccess && (grad || xcompact) && !na.compat) e = launch_num_prep(na, side->stream, &why);
  if (e == hipSuccess && !na.compat) e = launch_num_fb(na, side->stream, &why);
  if (e == hipSuccess && na.corrupt_b >= 0 && !na.compat) e = launch_num_corrupt(na, side->stream);
  if (e == hipSuccess && grad && !na.general && !na.compat) e = launch_num_occ(na, true, side->stream, &why);   // compact rows, off the critical path
  else if (e == hipSuccess && xcompact) {
    NumArgs nc = na;
    nc.bad = xc->scratch_bad;
    e = launch_num_occ(nc, true, side->stream, &why);
  }
  if (e == hipSuccess) e = hipEventRecord(side->join, side->stream);
  // the cross-entropy row kernel: on the side stream BEHIND the event the fold waits for - a memory-bound pass beside the
  // denominator's recursions -, joined to the caller's stream by an event of its own at the end of the call
  hipEvent_t xjoin = nullptr;
  if (e == hipSuccess && xcompact) {
    xjoin = xent_join_event(st);
    if (!xjoin) return fail(PYCHAIN_HIP_ELAUNCH, "%s: cannot create the xent event", who);
    e = run_xent(na, *xc, loss_norm_dev, side->stream, &why);
    if (e == hipSuccess) e = hipEventRecord(xjoin, side->stream);
  }
  da.phase_mask = da.knobs.den_phase_mask == 0 ? 0 : 3;     // (mask 0: only the numerator's launches - a measurement aid, outputs not meaningful)
  // (den_finish_kernel reads the numerator's objectives and its bad count for `totals`: the join precedes it)
  // (den_finish_kernel needs the numerator's objectives and bad count: early only where the occupancy launch waits for them)
  bool finished = fold;
  if (e == hipSuccess) e = run_den_launches(da, hint, grad != nullptr, st, &why, fold ? side->join : nullptr, side->fork, &finished);
  // join (a call whose occupancy launch folded the numerator in has it behind it already: that launch waited for the numerator's
  // event and the caller's stream for that launch - one barrier packet less, ~5 us, between it and den_finish_kernel)
  const bool joined = fold && da.phase_mask == 3;     // (every schedule of run_den_launches puts the wait in front of its first occupancy launch)
  if (e == hipSuccess && !joined) e = hipStreamWaitEvent(st, side->join, 0);
  if (e == hipSuccess && na.compat) e = launch_num_compat(na, grad ? 3 : 1, st);            // grad -= grad_scale * gamma_num, the reference's way
  if (e == hipSuccess && (da.phase_mask & 1) && !finished) e = launch_den_finish(da, st);     // (phase mask 0: the numerator alone - bench.py times it so)
  if (e == hipSuccess && grad && !fold && !na.compat)                               // grad -= grad_scale * gamma_num
    e = na.general ? launch_num_occ(na, false, st, &why) : launch_num_scatter(na, st, &why);
  if (e == hipSuccess && xjoin) e = hipStreamWaitEvent(st, xjoin, 0);
  if (e == hipSuccess && xc && na.general) e = run_xent(na, *xc, loss_norm_dev, st, &why);   // (dense posteriors: slow but complete)
  return e == hipSuccess ? PYCHAIN_HIP_OK : launch_failed(who, e, why);
}

// ---- a batch larger than the chip: slices (round 5).  From B = 224 on 256 CUs the recursion workgroups of ONE call (two
// sequences each: den_recursion_pair_kernel) hold every CU for the whole recursion, the numerator only finds room as they
// end, and the occupancy launch that folds it in starts late (DESIGN.md §4 "B >= 128": B = 256 11.1 ms against 2 x 5.06 for
// two calls of 128).  The fused call that also writes the gradient is therefore run over slices of about half the CU count
// in sequences, one after the other on the caller's stream, in the SAME workspaces; every slice reports into a scratch
// line at the end of the denominator's workspace, and one small launch sums the bad counts and forms `totals` from the
// per-sequence log-probabilities of the whole batch exactly as den_finish_kernel does (fp64, rounded once).
// Option chain_slices: 0 / 1 never, n >= 2 that many (where the batch allows), default automatic.
struct SliceLine { int32_t bad[2]; int32_t pad[2]; float totals[PYCHAIN_HIP_TOTALS]; };     // 48 bytes per slice
constexpr int kMaxSlices = 32;
__global__ void chain_slices_combine_kernel(const SliceLine* lines, int nslices, const float* den_objf, const float* num_objf,
                                            const int64_t* lengths, int B, int T, float loss_scale, const float* loss_norm_dev,
                                            int32_t* bad_count, float* totals) {
  __shared__ double part[2][4];
  double acc = 0.0, frames = 0.0;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    acc += (double)den_objf[i] - (double)num_objf[i];
    const int64_t l = lengths[i];
    frames += (double)(l < 1 ? 1 : (l > T ? T : l));
  }
  for (int o = 32; o > 0; o >>= 1) { acc += __shfl_down(acc, o); frames += __shfl_down(frames, o); }
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = acc; part[1][threadIdx.x >> 6] = frames; }
  __syncthreads();
  if (threadIdx.x == 0) {
    acc = (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
    frames = (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
    int b0 = 0, b1 = 0;
    float redone = 0.f, segs = 1.f, worst = 0.f;
    for (int c = 0; c < nslices; c++) {
      b0 += lines[c].bad[0]; b1 += lines[c].bad[1];
      redone += lines[c].totals[5]; segs = fmaxf(segs, lines[c].totals[6]); worst = fmaxf(worst, lines[c].totals[7]);
    }
    bad_count[0] = b0; bad_count[1] = b1;
    if (totals) {
      double t = acc * (double)loss_scale;
      if (loss_norm_dev) t /= (double)*loss_norm_dev;
      totals[0] = (float)t; totals[1] = (float)frames; totals[2] = (float)(b0 + b1); totals[3] = (float)acc; totals[4] = (float)t;
      totals[5] = redone; totals[6] = segs; totals[7] = worst;
    }
  }
}
// slices of a fused call over B sequences (1 = the call as it is)
int chain_loss_slices(int B, int hint, int64_t plan_stride_bytes, bool with_grad) {
  const int want = call_knobs().chain_slices;
  if (!with_grad || want == 0 || want == 1 || hint == PYCHAIN_HIP_HINT_GENERAL || plan_stride_bytes != 0) return 1;
  const int cus = device_cu_count();
  int n = 1;
  if (want >= 2) n = want;
  // automatic: slices of about CUs / 2 sequences, rather a few more than one slice more (measured on 256 CUs, profiles/r05_slices.txt:
  // B = 320 as 2 x 160 13.2 ms, as 3 x 107 13.8, one call 13.7; B = 384 as 3 x 128 15.6, as 2 x 192 17.0, one call 16.1)
  else if (8 * B >= 7 * cus) n = (int)(2.0 * B / cus + 0.25);
  n = std::min(n, std::min(kMaxSlices, B / 2));
  return std::max(n, 1);
}
}  // namespace

namespace {
// Which denominator workspaces were last written by a SLICED fused forward (every slice overwrote the one before it: only
// the last slice's trajectories are there, so pychain_hip_chain_loss_backward on them would write a wrong gradient for all
// earlier slices - ADVICE r5).  Host-side bookkeeping by workspace address, updated by every pychain_hip_chain_loss_forward.
std::mutex g_sliced_lock;
std::map<const void*, bool>& sliced_workspaces() { static std::map<const void*, bool> m; return m; }
void note_forward_workspace(const void* den_ws, bool sliced) {
  std::lock_guard<std::mutex> guard(g_sliced_lock);
  auto& m = sliced_workspaces();
  if (sliced) { if (m.size() > 256) m.clear(); m[den_ws] = true; } else m.erase(den_ws);
}
bool workspace_was_sliced(const void* den_ws) {
  std::lock_guard<std::mutex> guard(g_sliced_lock);
  return sliced_workspaces().count(den_ws) != 0;
}
}  // namespace

extern "C" int pychain_hip_chain_loss_slices(int64_t plan_stride_bytes, int hint, int B) {
  return chain_loss_slices(B, hint, plan_stride_bytes, true);
}

extern "C" int pychain_hip_chain_loss_forward_xent(
    const void* plans_dev, int64_t plan_stride_bytes, int hint, int den_H, float leaky,
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride, int num_H, int num_K,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    float* den_objf, float* num_objf, void* grad, float grad_scale, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_ws, size_t den_ws_bytes, void* num_ws, size_t num_ws_bytes, void* stream, const int32_t* time_windows,
    const pychain_hip_xent* xent) {
  XentCall xcall;
  if (xent) { if (int rc = xent_check(xent, B, T, num_H, num_K, D, "chain_loss_forward", xcall)) return rc; }
  const ChainLossCall c{{plans_dev, plan_stride_bytes, hint, den_H}, leaky,
                        {ft, fi, fp, bt, bi, bp, initial, final_, graph_batch_stride, num_H, num_K},
                        {nnet_output, nnet_output_dtype, seq_lengths, B, T, D},
                        den_objf, num_objf, grad, grad_scale, bad_count, loss_scale, loss_norm_dev, totals,
                        {den_ws, den_ws_bytes}, {num_ws, num_ws_bytes}, (hipStream_t)stream, time_windows, xent ? &xcall : nullptr};
  // the sums of the xent objectives and the full loss into totals[0], totals[4]: one small launch behind the call's last kernel
  auto xent_finish = [&]() -> int {
    if (!xent || (!xent->xent_totals && !totals)) return PYCHAIN_HIP_OK;
    const hipError_t xe = launch_xent_totals(xcall.objf, B, loss_scale, loss_norm_dev, xent->loss_coef, xent->xent_totals, totals, c.stream);
    if (xe != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "chain_loss_forward: %s", hipGetErrorString(xe));
    return PYCHAIN_HIP_OK;
  };
  const int nsl = (B > 0 && T > 0 && D > 0 && den_ws && bad_count && den_objf && num_objf && seq_lengths && nnet_output &&
                   !c.graphs.any_null() && den_ws_bytes > 8192)
                      ? chain_loss_slices(B, hint, plan_stride_bytes, grad != nullptr) : 1;
  note_forward_workspace(den_ws, nsl > 1);
  if (nsl <= 1) {
    const int rc1 = chain_loss_forward_one(c);
    return rc1 != PYCHAIN_HIP_OK ? rc1 : xent_finish();
  }
  // the scratch lines: the last 4 KiB of the denominator's workspace (sized by the caller for all B sequences; a slice
  // needs about 1 / nsl of it)
  const size_t ws_bytes = (den_ws_bytes - 4096) & ~(size_t)255;
  SliceLine* lines = reinterpret_cast<SliceLine*>((char*)den_ws + ws_bytes);
  // (a multiple of 8 sequences: every slice's rows, gradient and graph tensors start 16-byte aligned whatever T and D are -
  // 2-byte rows of odd T x D included -, and the pair recursion takes its sequences two by two)
  const int per = ((B + nsl - 1) / nsl + 7) & ~7;
  int n = 0;
  XentCall xslice;
  for (int b0 = 0; b0 < B; b0 += per, n++) {
    ChainLossCall s = c;                                     // the call over the sequences b0 .. b0 + per, reporting into its line
    s.graphs = c.graphs.at(b0); s.rows = c.rows.slice(b0, std::min(per, B - b0)); s.windows = window_row(time_windows, b0, num_H);
    s.den_objf = den_objf + b0; s.num_objf = num_objf + b0; s.grad = (char*)grad + c.rows.offset(b0);
    s.bad_count = lines[n].bad; s.totals = lines[n].totals; s.den_ws.bytes = ws_bytes;
    if (xent) { xslice = xent_slice(xcall, b0, T, D); s.xent = &xslice; }
    if (int rc = chain_loss_forward_one(s)) return rc;
  }
  hipLaunchKernelGGL(chain_slices_combine_kernel, dim3(1), dim3(256), 0, c.stream, lines, n, den_objf, num_objf, seq_lengths,
                     B, T, loss_scale, loss_norm_dev, bad_count, totals);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "chain_loss_forward: %s", hipGetErrorString(e));
  return xent_finish();
}

extern "C" int pychain_hip_chain_loss_forward_tw(
    const void* plans_dev, int64_t plan_stride_bytes, int hint, int den_H, float leaky,
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride, int num_H, int num_K,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    float* den_objf, float* num_objf, void* grad, float grad_scale, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_ws, size_t den_ws_bytes, void* num_ws, size_t num_ws_bytes, void* stream, const int32_t* time_windows) {
  return pychain_hip_chain_loss_forward_xent(plans_dev, plan_stride_bytes, hint, den_H, leaky, ft, fi, fp, bt, bi, bp, initial,
                                             final_, graph_batch_stride, num_H, num_K, nnet_output, nnet_output_dtype, seq_lengths, B, T, D,
                                             den_objf, num_objf, grad, grad_scale, bad_count, loss_scale, loss_norm_dev, totals, den_ws,
                                             den_ws_bytes, num_ws, num_ws_bytes, stream, time_windows, nullptr);
}

extern "C" int pychain_hip_chain_loss_forward(
    const void* plans_dev, int64_t plan_stride_bytes, int hint, int den_H, float leaky,
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride, int num_H, int num_K,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    float* den_objf, float* num_objf, void* grad, float grad_scale, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_ws, size_t den_ws_bytes, void* num_ws, size_t num_ws_bytes, void* stream) {
  return pychain_hip_chain_loss_forward_tw(plans_dev, plan_stride_bytes, hint, den_H, leaky, ft, fi, fp, bt, bi, bp, initial,
                                           final_, graph_batch_stride, num_H, num_K, nnet_output, nnet_output_dtype, seq_lengths, B, T, D,
                                           den_objf, num_objf, grad, grad_scale, bad_count, loss_scale, loss_norm_dev, totals, den_ws,
                                           den_ws_bytes, num_ws, num_ws_bytes, stream, nullptr);
}

// grad *= *scale_dev unless the scalar is exactly 1 (the common `loss.backward()` case costs one
// tiny launch; any other upstream gradient costs one pass over the buffer).
namespace {
__global__ void rescale_kernel(float4* data, size_t n4, float* tail, int ntail, const float* scale_dev) {
  const float g = *scale_dev;
  if (g == 1.0f) return;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 v = data[i];
    v.x *= g; v.y *= g; v.z *= g; v.w *= g;
    data[i] = v;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] *= g;
}
__global__ void rescale_half_kernel(uint32_t* data, size_t n2, uint16_t* tail, const float* scale_dev, int bf16) {
  const float g = *scale_dev;
  if (g == 1.0f) return;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
    float lo, hi;
    half2_to_f32(data[i], bf16 != 0, lo, hi);
    data[i] = pack_half2(lo * g, hi * g, bf16 != 0);
  }
  if (tail && blockIdx.x == 0 && threadIdx.x == 0) *tail = (uint16_t)f32_to_half_bits(half_bits_to_f32(*tail, bf16 != 0) * g, bf16 != 0);
}
}  // namespace

extern "C" int pychain_hip_rescale(void* data_, int dtype, size_t n, const float* scale_dev, void* stream) {
  if (!data_ || !scale_dev || ((uintptr_t)data_ & 15) || dtype < PYCHAIN_HIP_F32 || dtype > PYCHAIN_HIP_F16)
    return fail(PYCHAIN_HIP_EINVAL, "rescale: null or unaligned argument, or unknown dtype");
  if (dtype != PYCHAIN_HIP_F32) {                        // 2-byte gradients: value * scale in fp32, rounded to nearest even
    hipLaunchKernelGGL(rescale_half_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, (uint32_t*)data_, n / 2,
                       (n & 1) ? (uint16_t*)data_ + (n - 1) : nullptr, scale_dev, dtype == PYCHAIN_HIP_BF16 ? 1 : 0);
    hipError_t eh = hipGetLastError();
    if (eh != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "rescale: %s", hipGetErrorString(eh));
    return PYCHAIN_HIP_OK;
  }
  float* data = (float*)data_;
  const size_t n4 = n / 4;
  hipLaunchKernelGGL(rescale_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, (float4*)data, n4,
                     data + 4 * n4, (int)(n - 4 * n4), scale_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "rescale: %s", hipGetErrorString(e));
  return PYCHAIN_HIP_OK;
}

// out[0] = (sum den_objf - sum num_objf) * scale [/ *norm_dev]: the scalar of ChainLoss.forward (loss.py:100-104) in ONE
// launch instead of two reductions, a subtraction and a scaling of the host framework (each ~6 us, launch-bound, in the
// serial tail of every step).  fp64 accumulation, one rounding.
namespace {
__global__ void loss_total_kernel(const float* den, const float* num, int B, float scale, const float* norm_dev, float* out) {
  __shared__ double part[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < B; i += blockDim.x) acc += (double)den[i] - (num ? (double)num[i] : 0.0);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = ((part[0] + part[1]) + (part[2] + part[3])) * (double)scale;
    if (norm_dev) t /= (double)*norm_dev;
    out[0] = (float)t;
  }
}
}  // namespace

extern "C" int pychain_hip_loss_total(const float* den_objf_per_seq, const float* num_objf_per_seq, int B, float scale,
                                      const float* norm_dev, float* out, void* stream) {
  if (!den_objf_per_seq || !out || B <= 0) return fail(PYCHAIN_HIP_EINVAL, "loss_total: null pointer or empty batch");
  hipLaunchKernelGGL(loss_total_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, den_objf_per_seq, num_objf_per_seq, B, scale,
                     norm_dev, out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "loss_total: %s", hipGetErrorString(e));
  return PYCHAIN_HIP_OK;
}

extern "C" int pychain_hip_chain_loss_backward(
    const void* plans_dev, int64_t plan_stride_bytes, int hint, int den_H,
    const int32_t* ft, const int32_t* fi, const float* fp, int graph_batch_stride, int num_H, int num_K,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D,
    float grad_scale, const float* grad_scale_dev, void* grad, int32_t* bad_count,
    void* den_ws, size_t den_ws_bytes, void* num_ws, size_t num_ws_bytes, void* stream) {
  const char* who = "chain_loss_backward";
  const Rows rows{nnet_output, nnet_output_dtype, seq_lengths, B, T, D};
  if (!bad_count || !ft || !fi || !fp) return null_pointer(who);
  if (workspace_was_sliced(den_ws))
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: the forward call on these workspaces wrote its gradient in slices (a batch larger than the "
                "chip: pychain_hip_chain_loss_slices) - the workspaces hold the last slice's trajectories only.  Take the gradient "
                "that call wrote, or call pychain_hip_chain_loss_forward without a gradient first", who);
  DenArgs da;
  float dummy_coef = 0.5f;       // the occupancy launch does not use the leaky coefficient
  if (nnet_output_dtype != PYCHAIN_HIP_F32)              // (the numerator's occupancy launch accumulates into an fp32 gradient)
    return fail(PYCHAIN_HIP_EUNSUPPORTED, "%s: 2-byte network outputs are taken by the forward call that also writes the gradient", who);
  if (int rc = fill_den_args(da, DenPlan{plans_dev, plan_stride_bytes, hint, den_H}, rows, 0, dummy_coef, grad_scale, (float*)den_ws, grad,
                             bad_count, Workspace{den_ws, den_ws_bytes}, who)) return rc;
  da.grad_scale_dev = grad_scale_dev;
  da.fused = 1;                                          // (the forward call that stored the rows decided as a fused call)
  den_decide_family(da, hint);                           // (what the stored rows ARE: DenArgs::lazy, DenArgs::sg)
  NumArgs na;
  // the occupancy launch reads only the forward transitions / indices / log-probs of the graphs
  if (int rc = fill_num_args(na, NumGraphs{ft, fi, fp, ft, fi, fp, fp, fp, graph_batch_stride, num_H, num_K}, rows, PYCHAIN_HIP_GRAD_ACCUM,
                             -grad_scale, (float*)num_ws, grad, bad_count + 1, Workspace{num_ws, num_ws_bytes}, who, nullptr)) return rc;   // (stored rows: no windows)
  na.grad_scale_dev = grad_scale_dev;
  hipStream_t st = (hipStream_t)stream;
  const char* why = nullptr;
  hipError_t e = hipMemsetAsync(bad_count, 0, 2 * sizeof(int32_t), st);
  da.phase_mask = 2;
  if (e == hipSuccess)
    e = hint == PYCHAIN_HIP_HINT_GENERAL ? launch_den_general(da, st) : launch_den(da, (D + 63) / 64, hint, st, &why);
  if (e == hipSuccess) e = na.compat ? launch_num_compat(na, 2, st) : launch_num_occ(na, false, st, &why);
  return e == hipSuccess ? PYCHAIN_HIP_OK : launch_failed(who, e, why);
}

extern "C" int pychain_hip_chain_loss_forward_backward_xent(
    const void* plans_dev, int64_t plan_stride_bytes, int hint, int den_H, float leaky,
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride, int num_H, int num_K,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D, float grad_scale,
    float* den_objf, float* num_objf, void* grad, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_ws, size_t den_ws_bytes, void* num_ws, size_t num_ws_bytes, void* stream, const int32_t* time_windows,
    const pychain_hip_xent* xent) {
  if (!grad) return fail(PYCHAIN_HIP_EINVAL, "chain_loss_forward_backward: null grad");
  return pychain_hip_chain_loss_forward_xent(plans_dev, plan_stride_bytes, hint, den_H, leaky, ft, fi, fp, bt,
                                             bi, bp, initial, final_, graph_batch_stride, num_H, num_K, nnet_output, nnet_output_dtype,
                                             seq_lengths, B, T, D, den_objf, num_objf, grad, grad_scale, bad_count, loss_scale,
                                             loss_norm_dev, totals, den_ws, den_ws_bytes, num_ws, num_ws_bytes, stream, time_windows, xent);
}

extern "C" int pychain_hip_chain_loss_forward_backward_tw(
    const void* plans_dev, int64_t plan_stride_bytes, int hint, int den_H, float leaky,
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride, int num_H, int num_K,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D, float grad_scale,
    float* den_objf, float* num_objf, void* grad, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_ws, size_t den_ws_bytes, void* num_ws, size_t num_ws_bytes, void* stream, const int32_t* time_windows) {
  return pychain_hip_chain_loss_forward_backward_xent(plans_dev, plan_stride_bytes, hint, den_H, leaky, ft, fi, fp, bt, bi, bp,
                                                      initial, final_, graph_batch_stride, num_H, num_K, nnet_output, nnet_output_dtype,
                                                      seq_lengths, B, T, D, grad_scale, den_objf, num_objf, grad, bad_count, loss_scale,
                                                      loss_norm_dev, totals, den_ws, den_ws_bytes, num_ws, num_ws_bytes, stream, time_windows, nullptr);
}

extern "C" int pychain_hip_chain_loss_forward_backward(
    const void* plans_dev, int64_t plan_stride_bytes, int hint, int den_H, float leaky,
    const int32_t* ft, const int32_t* fi, const float* fp, const int32_t* bt, const int32_t* bi, const float* bp,
    const float* initial, const float* final_, int graph_batch_stride, int num_H, int num_K,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int D, float grad_scale,
    float* den_objf, float* num_objf, void* grad, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_ws, size_t den_ws_bytes, void* num_ws, size_t num_ws_bytes, void* stream) {
  return pychain_hip_chain_loss_forward_backward_tw(plans_dev, plan_stride_bytes, hint, den_H, leaky, ft, fi, fp, bt, bi, bp,
                                                    initial, final_, graph_batch_stride, num_H, num_K, nnet_output, nnet_output_dtype,
                                                    seq_lengths, B, T, D, grad_scale, den_objf, num_objf, grad, bad_count, loss_scale,
                                                    loss_norm_dev, totals, den_ws, den_ws_bytes, num_ws, num_ws_bytes, stream, nullptr);
}

// ---- on-device reorder of a staged batch (include/pychain_hip.h: batch containers) ------------------------------------
namespace {
struct GatherArgs { int64_t in_off[PYCHAIN_HIP_BATCH_FIELDS], out_off[PYCHAIN_HIP_BATCH_FIELDS], row_bytes[PYCHAIN_HIP_BATCH_FIELDS]; };
__global__ void batch_gather_kernel(const char* in, char* out, const int64_t* order, int B_in, GatherArgs g) {
  const int b = blockIdx.x, f = blockIdx.y;
  const int64_t rb = g.row_bytes[f];
  if (rb == 0) return;
  int64_t src = order[b];
  if (src < 0 || src >= B_in) src = 0;                                    // (validated on the host where the order lives there)
  const uint32_t* s = reinterpret_cast<const uint32_t*>(in + g.in_off[f] + rb * src);
  uint32_t* d = reinterpret_cast<uint32_t*>(out + g.out_off[f] + rb * b);
  for (int64_t i = threadIdx.x; i < rb / 4; i += blockDim.x) d[i] = s[i];
}
}  // namespace
extern "C" int pychain_hip_batch_reorder_dev(int B_in, int B_out, int K, int H, int log_domain, const void* in_dev, void* out_dev,
                                             const int64_t* order_dev, void* stream) {
  GatherArgs g;
  if (pychain_hip_batch_layout(B_in, K, H, log_domain, g.in_off, g.row_bytes) < 0 ||
      pychain_hip_batch_layout(B_out, K, H, log_domain, g.out_off, g.row_bytes) < 0)
    return PYCHAIN_HIP_EINVAL;
  if (!in_dev || !out_dev || !order_dev) return fail(PYCHAIN_HIP_EINVAL, "batch_reorder_dev: null pointer");
  hipLaunchKernelGGL(batch_gather_kernel, dim3(B_out, PYCHAIN_HIP_BATCH_FIELDS), dim3(256), 0, (hipStream_t)stream,
                     (const char*)in_dev, (char*)out_dev, order_dev, B_in, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PYCHAIN_HIP_ELAUNCH, "batch_reorder_dev: %s", hipGetErrorString(e));
  return PYCHAIN_HIP_OK;
}
