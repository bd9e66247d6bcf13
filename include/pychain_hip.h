/*
 * pychain_hip.h - C ABI of libpychain_hip.so, the MI355X (gfx950) LF-MMI
 * forward-backward.  This library replaces the reference's native extension
 * `pychain_C` (pytorch_binding/src, built by pytorch_binding/setup.py:4-14)
 * wholesale.  Plain pointers and sizes only: no torch / pybind types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative PYCHAIN_HIP_E* code on
 *     error; pychain_hip_last_error() then holds a message (thread-local);
 *   - "dev" pointers are device memory, "host" pointers host memory;
 *   - all work is ordered on the caller's stream (`void* stream` is a hipStream_t):
 *     a call may fork launches to two library-owned non-blocking side streams
 *     (created once per device on first use - with their events the only hidden
 *     state of the library) and joins them back with events before it returns, so
 *     stream-ordered use is unchanged.  The denominator does this for T >= 256: its
 *     time-parallel occupancy launches run beside the (single) recursion launch,
 *     each released by a one-wave gate kernel that polls a progress counter the
 *     recursion workgroups advance.  Nothing synchronises with the
 *     host and nothing allocates: scratch memory is a caller-provided workspace
 *     sized by the *_workspace_bytes queries;
 *   - float = IEEE fp32, indices int32, lengths int64 (the reference's dtypes,
 *     openfst_binding/src/fstext.cc:81-104, pychain/loss.py:41).
 *
 * Reference boundary being replaced (pytorch_binding/src/pychain.cc):
 *   pychain_C.forward_backward            :26-79   -> pychain_hip_den_*  (probability domain, leaky-HMM)
 *   pychain_C.forward_backward_log_domain :81-129  -> pychain_hip_num_*  (log domain)
 *   pychain_C.set_verbose_level           :134     -> pychain_hip_set_verbose_level
 */
#ifndef PYCHAIN_HIP_H_
#define PYCHAIN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYCHAIN_HIP_ABI_VERSION 32

/* Element type of the network output [B,T,D] - and of the gradient an entry point writes for it (ABI 14).
 * 2-byte rows are read as they are by the kernels and converted where they land; the gradient is rounded (to nearest even)
 * to the same type where it is written: no up-cast pass, no fp32 copy of [B,T,D], no cast of the gradient back.  All
 * arithmetic is fp32 (fp64 for the numerator's log-probabilities) whatever the storage type.  Not every kernel family takes
 * 2-byte rows: ask pychain_hip_*_half_native first (a call that cannot returns PYCHAIN_HIP_EUNSUPPORTED; up-cast then). */
#define PYCHAIN_HIP_F32  0
#define PYCHAIN_HIP_BF16 1
#define PYCHAIN_HIP_F16  2

#define PYCHAIN_HIP_OK            0
#define PYCHAIN_HIP_EINVAL      (-1)  /* bad argument (null pointer, size mismatch, index out of range) */
#define PYCHAIN_HIP_EUNSUPPORTED (-2) /* shape outside what the kernels were built for */
#define PYCHAIN_HIP_EWORKSPACE  (-3)  /* workspace / blob too small */
#define PYCHAIN_HIP_ELAUNCH     (-4)  /* HIP runtime reported a launch error */

int         pychain_hip_abi_version(void);
const char* pychain_hip_last_error(void);
/* base.h:34-42 / pychain.cc:134.  `ok` (here: bad_count == 0) carries the reference's invariant checks
 * (chain-computation.cc:345-391, chain-log-domain-computation.cc:283-304): alpha'.beta' and the frame's
 * derivative sum within 5 % of 1, restated for this library's free per-frame scales as
 *   log G(t) + la[t] + lb[t+2] = log P(sequence)   (denominator; G = un-normalised occupancy total of frame t,
 *   la / lb = log-scales the two recursions have divided out), sum of a frame's occupancies = 1 (numerator),
 * plus: no normaliser or total is non-finite or non-positive.  Level 0 checks frame 0 of every sequence (as the
 * reference does), level >= 1 every frame; at level >= 1 the occupancy launches of the denominator are not
 * overlapped with the recursions (the check needs both finished), results are bit-identical. */
void        pychain_hip_set_verbose_level(int level);
int         pychain_hip_get_verbose_level(void);

/* Test hook (host only, no GPU): how the occupancy launch of time segment `seg` (of `nseg`, ends
 * seg_bound[]) maps workgroups to 32-frame chunks of a length-L sequence.
 * out[0] = grid.x, out[1 + k] = chunk of workgroup k or -1; returns 1 if frame t belongs to the
 * launch, 0 if not, negative on bad arguments.  nseg = 0: the unsegmented launch. */
int         pychain_hip_debug_launch_map(int T, int L, int t, int frames_per_block, int nseg,
                                         const int32_t* seg_bound, int seg, int32_t* out, int out_len);
/* Test hook (host only, no GPU): the rings of the STREAMED occupancy pass for sequences of up to T frames:
 * ring r covers the frames whose step count need = max(t, L-1-t) lies in [out[2r], out[2r+1]); returns the number of rings
 * (pairs beyond out_len / 2 are not written).  report_due (may be NULL): report_due[d] = 1 if a recursion workgroup reports its
 * progress after d steps, d < due_len. */
int         pychain_hip_debug_stream_rings(int T, int32_t* out, int out_len, int32_t* report_due, int due_len);
/* Test hook: `workgroups` workgroups of 1024 threads and 100 KB of LDS (one to a CU) that sleep for `microseconds` on `stream` -
 * a stand-in for the long-lived kernels of an overlapped RCCL all-reduce beside a loss step (tests/test_gpu_robust.py). */
int         pychain_hip_debug_occupy(int workgroups, int microseconds, void* stream);
/* Measurement aid (bench.py): restrict pychain_hip_den_forward_backward to a subset of
 * its launches so each kernel can be bracketed by events on the caller's stream.
 * bit 0 = alpha/beta recursion launch, bit 1 = occupancy launch; default 3 = both.
 * With a partial mask the outputs of the call are NOT meaningful. */
void        pychain_hip_set_den_phase_mask(int mask);
/* Test hook: 0 = the denominator recursions always run as den_recursion_kernel (rows normalised in a
 * pass of their own, two barriers per frame); 1 (default) = as den_recursion_lazy_kernel wherever the
 * shape allows.  Both forms must agree to rounding; the tests compare them. */
void        pychain_hip_set_den_lazy(int on);
/* Which kernels a denominator call with this plan hint (pychain_hip_den_plan_info: info[4]), these sizes and the
 * calling thread's current options would launch: "recursion,occupancy" into buf, e.g.
 * "den_recursion_lazy_kernel<dma>,den_gamma2_kernel".  Recursion: den_recursion_lazy_kernel<small> (4 waves: plans that
 * hold the four-wave dealing), den_recursion_lazy_kernel<dma> (16 waves, nnet-output rows of up to 9216 pdfs by LDS-direct
 * loads), den_recursion_lazy_kernel (16 waves, rows through registers: option den_dma = 0), den_recursion_pair_kernel (two
 * sequences per workgroup, shared plan, B >= 3/8 of the CU count), den_recursion_kernel (everything else),
 * den_general_recursion_kernel (plans in the general format).  Measurement tools and the kernel-selection test label by it.
 * plans_shared: bit 0 = one plan for all sequences (plan stride 0); bit 1 = the call is a fused loss (a numerator runs beside
 * it: two sequences per recursion workgroup from B >= 100 on 256 CUs; the denominator alone: once 2 B workgroups no longer fit). */
int         pychain_hip_den_kernel_names(int resident_slot_rows, int num_states, int num_pdfs, int B, int plans_shared,
                                         char* buf, size_t buf_bytes);
/* Settings.  A call reads them ONCE when it starts (process-wide defaults overlaid with the calling thread's
 * overrides), so another thread changing one cannot tear a call in flight, and nothing on the call path reads the
 * environment.  pychain_hip_set_option sets the process-wide default (value NULL or "" clears it);
 * pychain_hip_set_thread_option overrides it for the calling host thread only (value NULL removes the override,
 * "" = unset for this thread); pychain_hip_get_option copies the value in effect for the calling thread into buf and
 * returns its length (0 = unset).  pychain_hip_set_verbose_level / _set_den_phase_mask / _set_den_lazy are the
 * process-wide "verbose" / "den_phase_mask" / "den_lazy".  The thirteen names - every one selects between SHIPPED kernel
 * families so that the tests can compare them (all give the same results to rounding; most bit for bit), or is a test hook:
 *   "verbose"        base.h:34-42: >= 1 checks the reference's invariant on every frame instead of frame 0
 *   "den_phase_mask" bit 0 recursion launch, bit 1 occupancy launch (measurement aid)
 *   "den_lazy"       "0": the two-barrier recursion (den_recursion_kernel) instead of the lazy-normalisation one
 *   "den_dma"        "0": nnet-output rows of the lazy recursion through registers instead of LDS-direct loads; "2": LDS-direct,
 *                    and the recursions clamp / exp every row themselves instead of gathering from rows den_exp_rows_kernel
 *                    exp'd ahead of them on the side stream (bit-identical); "3": rows exp'd ahead wherever the shape allows - by
 *                    default only four-wave workgroups take them
 *   "den_segments"   n >= 1: the occupancy pass in n gated time segments (1 = after the recursions, no overlap) instead of
 *                    the streamed persistent launch
 *   "den_pair"       "1": two sequences per recursion workgroup wherever the shape allows, "0": never; default: a fused loss from 25/64
 *                    of the CU count in sequences on (B >= 100 on 256 CUs), the denominator alone once 2 B one-sequence
 *                    workgroups no longer fit the chip (B > 128) - bit-identical to den_recursion_kernel
 *   "gamma16"        the one-frame occupancy kernel (and with it the numerator accumulated into the stored gradient
 *                    instead of folded into the occupancy launch) also where the two-frame kernel fits
 *   "debug_corrupt_row" "den,b,t,scale" / "num,b,t,scale": the stored alpha row t of sequence b is scaled between the
 *                    recursions and the occupancy pass, so that the 5 % invariant of chain-computation.cc:363-390 /
 *                    chain-log-domain-computation.cc:289-303 can be seen to fire: `ok` false at t = 0, at any t at verbose >= 1
 *   "num_compat"     "1": the numerator in the reference's own fp32 arithmetic (num_compat.hip) instead of the exact path
 *   "den_tseg"       time segments per (sequence, direction) of the lazy recursions: unset / "-1" automatic (few sequences
 *                    only: pychain_hip_den_time_segments), "0": never, "2" / "4": wherever the shape allows
 *   "den_tburn"      frames a time segment starts outside itself (default 192); see totals[5..7] and pychain_hip_den_tseg_state
 *   "den_sg"         "0": a "pdf by state" plan (every arc entering a state carries one pdf: pychain_hip_den_plan_info, hint bit 27) runs
 *                    the recursions every plan runs instead of their one-gather form (the tests compare the two)
 *   "den_q"          "1": the lazy recursions keep ONE-WORD state vectors where the plan allows them (every leaky probability
 *                    positive, one position per state: pychain_hip_den_plan_info, hint bit 19; fp32 rows, uncut sequences, loops of
 *                    17 .. 32 slot-rows): alpha gathers a / (coef leaky), both directions two ds_read_b32 per arc instead of a
 *                    ds_read_b64 and a ds_read_b32.  Off by default: a third fewer LDS bytes per gather pair, same results to 3e-7 - and
 *                    measured 6 % slower with rows the recursions clamp / exp themselves, 7 % faster with rows exp'd ahead (the
 *                    LDS pipe is as busy as before - a b64 gather occupies it about as long as a b32 one - and the group ends add 12 %
 *                    VALU: DESIGN.md 3.16, profiles/r06_one_word_states.txt)
 *   "den_cross"      "1": the recursions of a pdf-by-state plan emit occupancies themselves (calls of the denominator alone with at
 *                    most one workgroup per CU: each direction emits those of its own second half, the occupancy launch handles the
 *                    band around every middle).  Off by default: same results to 3e-7, but measured slower than the streamed
 *                    occupancy launch it replaces (profiles/r06_crossing.txt).  Each direction waits for rows of
 *                    the other, so every workgroup of the launch must be resident: not beside other work on the same GPU (a
 *                    workgroup that waits 20 s for its peer gives up and the call reports `ok` false)
 *   "chain_slices"   the fused loss with a gradient over a batch larger than the chip: "0" one call, "n" n slices; default automatic
 *   "plan_split"     read by pychain_hip_den_plan_build: "0": no state on more than one lane; default: where it gains a
 *                    shorter register-resident loop
 * Unknown name: EINVAL.  (Kernel variants that measured slower - 8 / 12 waves, two copies of the nnet-output row, a
 * recursion relaunched per segment - are not in the library; their measurements are under profiles/r03_*.) */
int         pychain_hip_set_option(const char* name, const char* value);
int         pychain_hip_set_thread_option(const char* name, const char* value);
int         pychain_hip_get_option(const char* name, char* buf, size_t buf_bytes);

/* ------------------------------------------------------------------------
 * Denominator graph plan  (host side, no GPU work).
 *
 * Compiles ONE probability-domain graph, given in the reference layout
 * (pychain/graph.py:36-44; fstext.cc:49-116), into the device format the
 * kernels consume: three degree-sorted, wave-tiled arc orderings
 *   by destination state (alpha recursion; = reference backward_transitions),
 *   by source state      (beta recursion;  = reference forward_transitions),
 *   by pdf-id            (occupancy pass;  replaces the reference's atomicAdd
 *                         scatter, chain-kernels.cu:53-87,230-240)
 * plus the permuted leaky / initial / final vectors.
 *
 * States on several lanes: a row group of a recursion is as long as its longest row, so one state with many arcs
 * entering (leaving) it would set the loop length of the whole workgroup.  Where it gains a shorter register-resident loop
 * the compiler puts such a state on several POSITIONS of a side's numbering, each collecting a share of its arcs; the
 * arcs that gather the state are repeated once per position (csrc/plan.cpp).  The plan then has more positions than the
 * graph has states: pychain_hip_den_plan_info reports the position count as info[0] - THE VALUE TO PASS AS num_states
 * to the workspace and forward-backward calls - and the graph's own count as info[6].  Results are the same to rounding.
 * Plans passed to one call with a non-zero stride must agree in info[0]: build them with the option "plan_split" = "0"
 * (no state on more than one lane).
 *
 * Graphs the tile kernels do not take - more than 65 535 states or pdfs (packed 16-bit arc addresses), or a state
 * vector + nnet-output row beyond the 160 KiB LDS of one CU - are compiled into a GENERAL format instead (the reference
 * layout plus the arcs grouped by pdf-id); pychain_hip_den_plan_info then reports the launch hint
 * PYCHAIN_HIP_HINT_GENERAL and the denominator runs on kernels that gather from global memory: slow, but complete,
 * like the reference's CPU path (chain-computation.cc:113-176,247-311 has no size limit).
 *
 * Returns the number of bytes the plan needs (> 0).  If `blob` is NULL or
 * `blob_bytes` is too small nothing is written (call once to size, once to
 * fill).  The filled blob is position independent: copy it to the device with
 * any allocator and pass the device address to pychain_hip_den_forward_backward.
 * Negative return = error.
 */
int64_t pychain_hip_den_plan_build(
    const int32_t* forward_transitions,        /* host [K,3] (src,dst,pdf)          */
    const int32_t* forward_transition_indices, /* host [H,2] (begin,end) by source   */
    const float*   forward_transition_probs,   /* host [K]   probabilities           */
    const int32_t* backward_transitions,       /* host [K,3] grouped by destination  */
    const int32_t* backward_transition_indices,/* host [H,2]                         */
    const float*   backward_transition_probs,  /* host [K]                           */
    const float*   leaky_probs,                /* host [H]                           */
    const float*   initial_probs,              /* host [H]                           */
    const float*   final_probs,                /* host [H]                           */
    int num_states, int num_transitions, int num_pdfs,
    void* blob, size_t blob_bytes);

/* Facts about a filled HOST blob that the launcher needs (the blob itself lives on the
 * device at call time and is never read back):
 *   info[0] num_states (positions: see "States on several lanes")  info[1] num_transitions  info[2] num_pdfs  info[3] plan bytes, low 31 bits (info[5]: the rest)
 *   info[4] launch hint: slot-rows per wave (= arcs a wave keeps in registers), three
 *           fields: recursion plans (bits 0-9), occupancy plan for 16 waves (10-18; ABI 17: nine bits)
 *           and for 8 waves (20-27); combine several plans by taking the max of each field
 *           bit 19: (ABI 17) every state sits on one position of either numbering and every leaky probability is positive: the
 *                   lazy recursions may keep ONE-WORD state vectors (alpha gathers a / (coef leaky); option "den_q") (AND)
 *           bit 28: a state sits on several positions of the beta numbering: the lazy recursions' NC form; not for
 *                   den_recursion_pair_kernel (OR)
 *           bit 29: the plan also holds its recursion tiles dealt to FOUR waves (small graphs: 256-thread recursion
 *                   workgroups); the recursion field is then that dealing's row count (AND over several plans)
 *           bit 30: every recursion wave owns few enough row groups for the lazy-normalisation recursions (AND)
 *   info[5] plan bytes >> 31 (general-format plans may exceed 2 GiB)   info[6] the graph's states, info[7] positions
 *   added by states on several lanes (0: none)
 * A blob whose header or payload does not match the checksums in its header, or whose header points outside the blob
 * (a damaged or foreign cache file), is EINVAL.
 */
int pychain_hip_den_plan_info(const void* host_blob, size_t blob_bytes, int32_t info[8]);

/* ------------------------------------------------------------------------
 * Denominator forward-backward on the GPU (replaces pychain.cc:26-79 and all
 * of chain-computation.cc / chain-kernels.cu).
 *
 * plans_dev/plan_stride_bytes: device address of the first plan and the byte
 *   distance between the plans of consecutive sequences; 0 = every sequence
 *   shares one graph (the ChainLoss denominator, pychain/loss.py:99).
 * resident_slot_rows: the launch hint info[4] of pychain_hip_den_plan_info (per-field max
 *   over the passed plans); selects the kernel variant that keeps every wave's arcs
 *   in registers for the whole launch.  0 = unknown (arcs are re-read from L2 each frame;
 *   same results, slower).
 * nnet_output: dev [B,T,D].  input_is_exp = 0: raw network output, clamp(-30,30)
 *   and exp are fused into the kernels (pychain/loss.py:30,43);
 *   input_is_exp = 1: already exp(clamp(.)) as pychain_C.forward_backward gets it.
 * seq_lengths: dev [B] int64, 1 <= len <= T.  Any order (the reference needs
 *   them sorted descending for pack_padded_sequence, loss.py:37-40).
 * objf_per_seq: dev [B], log-probability of each sequence (reference returns
 *   their sum, chain-computation.cc:229).
 * grad: dev [B,T,D], d objf / d nnet_output, every element written (rows
 *   t >= len are zero), multiplied by grad_scale.
 * bad_count: dev int32[1]; zeroed by the call, incremented by every frame or
 *   sequence whose normaliser is not finite-positive (the reference's `ok`
 *   flag, chain-computation.cc:367-390, without a host sync).
 * totals: dev float[PYCHAIN_HIP_TOTALS = 8] or NULL.  The call's last kernel adds up what a caller otherwise computes in several
 *   launch-bound scalar kernels behind it (the reference: `tot_log_prob.sum()`, chain-computation.cc:229):
 *   totals[0] = totals[3] = sum_b objf_per_seq[b] (fp64 accumulation, rounded once), totals[1] = sum_b len_b,
 *   totals[2] = bad_count as a float; totals[4] = totals[0] once more (ABI 14: the scalar a host framework hands out as the
 *   loss, apart from the statistics in [0..3] that it may all-reduce or keep); totals[5] = speculated rows of a time-segmented
 *   call that did not verify (0, or the call ran its recursions again unsegmented), totals[6] = its segments per (sequence,
 *   direction) (1: not segmented), totals[7] = the worst mismatch of a speculated row q against the true row p, per state: max_i |q_i - c p_i| / (c p_i) with
 *   c = sum q / sum p (the bound is 9e-6 / (2 (segments - 1)): 4.5e-6 for two segments, 1.5e-6 for four; +inf where a row is dead
 *   or only one of the two has a state at zero).
 * workspace: the stored alpha' / beta rows (4 B T roundup64(num_states) bytes each), per-frame totals, counters, and - in a
 *   call of the denominator alone - a [B,T,D] buffer for the rows exp'd ahead of the recursions (den_exp_rows_kernel: C4
 *   4.80 -> 4.57 ms): pychain_hip_den_workspace_bytes; pychain_hip_den_workspace_min_bytes is the size without it.
 */
#define PYCHAIN_HIP_TOTALS 8
size_t pychain_hip_den_workspace_bytes(int B, int T, int num_states, int num_pdfs);
/* ... without the [B,T,D] buffer: a workspace of at least this size is accepted everywhere; the rows are then never exp'd
 * ahead (the fused loss never does: its callers pass this size). */
size_t pychain_hip_den_workspace_min_bytes(int B, int T, int num_states, int num_pdfs);
/* 1 if pychain_hip_den_forward_backward with these arguments (and the calling thread's options) would use the [B,T,D] buffer
 * of the full workspace, else 0: a caller that caches its workspace asks before it allocates as much again as the network
 * output (1.3 GB at C3) for calls that never touch it (pair / general / two-barrier kernels, T < 64, exp'd input, a recursion
 * grid that leaves less than a quarter of the chip free). */
/* How many time segments the recursions of a (sequence, direction) of such a call are cut into (1: not cut; `fused`: the
 * call is a fused loss - a quarter of the chip stays with the numerator).  totals[5..7] of the call report how the cut went.
 * A function of the shape, the device's CU count and the options den_tseg / den_tburn only - NOT of the verbose level (a debug
 * run computes what production computes).  A cut call's results differ from the uncut call's within the fp32 noise of two
 * recursions (objf bit-equal, gradient ~2e-7), and which shapes are cut depends on B and the CU count: option den_tseg = "0" is
 * the ONE switch for training that must reproduce bit for bit across batch shapes and devices. */
int pychain_hip_den_time_segments(int64_t plan_stride_bytes, int resident_slot_rows, int num_states, int num_pdfs, int B, int T, int fused);
/* The burn-in controller of a plan (ABI 16).  How long a recursion needs to forget where it started depends on
 * the DATA (peaky network outputs forget slowly), and a call whose speculated rows do not verify runs its recursions twice.
 * state_dev: pychain_hip_den_tseg_state_bytes() (64) bytes of DEVICE memory the caller owns and has zeroed ONCE; attached to the
 * plan by address (NULL detaches; detach before freeing either).  Every time-segmented call on that plan then reads its burn-in
 * from the state and the call's last kernel updates it - in stream order, on the device: after a call that missed, the burn-in
 * is half as long again while three of them fit T; beyond that the plan is not cut for the next 500 calls (the segmented launch
 * leaves at once, the uncut launch behind it does the work) and starts over from the default.  No host read, no host timing:
 * the burn-in of call n is a function of the calls before it on the stream - the same run gives the same bits.  Callers that
 * pin "den_tseg" or "den_tburn" with an option bypass the state.  int32 words: [0] magic, [1] burn-in, [2] cool-down calls left,
 * [3] calls seen, [4] calls that missed.  One state per plan AND stream if calls on one plan overlap on several streams. */
int pychain_hip_den_tseg_state(const void* plans_dev, void* state_dev);
size_t pychain_hip_den_tseg_state_bytes(void);
int pychain_hip_den_uses_row_buffer(int64_t plan_stride_bytes, int resident_slot_rows, int num_states, int num_pdfs,
                                    int B, int T, int input_is_exp);
int pychain_hip_den_forward_backward(
    const void* plans_dev, int64_t plan_stride_bytes, int resident_slot_rows,
    int num_states, int num_pdfs,
    const void* nnet_output, int nnet_output_dtype, int input_is_exp, const int64_t* seq_lengths,
    int B, int T, float leaky_hmm_coefficient, float grad_scale,
    float* objf_per_seq, void* grad /* nnet_output_dtype */, int32_t* bad_count, float* totals,
    void* workspace, size_t workspace_bytes, void* stream);
/* 1 if pychain_hip_den_forward_backward takes 2-byte network outputs for this shape (and the calling thread's options): the
 * lazy recursions with LDS-direct rows or the pair recursion, an occupancy kernel in its float4-chunk forms, rows of a
 * multiple of 8 pdfs, a plan that is not in the general format. */
int pychain_hip_den_half_native(int64_t plan_stride_bytes, int resident_slot_rows, int num_states, int num_pdfs, int B, int T);

/* ------------------------------------------------------------------------
 * Numerator forward-backward, log domain, one graph per sequence (replaces
 * pychain.cc:81-129 and chain-log-domain-computation.cc / -kernels.cu).
 * Graph tensors are the batched, zero-padded ChainGraphBatch tensors
 * (pychain/graph.py:122-175) already on the device; graph_batch_stride = 1
 * for per-sequence graphs, 0 when all sequences share row 0.
 * nnet_output: dev [B,T,D] raw (clamped to [-30,30] in-kernel).
 * grad_mode:
 *   PYCHAIN_HIP_GRAD_LOG    grad[b,t,n] = log occupancy, -inf where zero (what
 *                           forward_backward_log_domain returns, :57,:265)
 *   PYCHAIN_HIP_GRAD_LINEAR grad[b,t,n] = grad_scale * occupancy (loss.py:77 fused)
 *   PYCHAIN_HIP_GRAD_ACCUM  grad[b,t,n] += grad_scale * occupancy on the touched
 *                           pdfs only (fused ChainLoss: pass grad_scale < 0 to
 *                           subtract the numerator from the denominator grad)
 */
#define PYCHAIN_HIP_HINT_GENERAL ((int)0x80000000)   /* launch hint of a plan in the general format (pychain_hip_den_plan_info) */
#define PYCHAIN_HIP_GRAD_LOG    0
#define PYCHAIN_HIP_GRAD_LINEAR 1
#define PYCHAIN_HIP_GRAD_ACCUM  2
/* pychain_hip_cpu_num_forward_backward only, OR-ed into grad_mode: the network output is taken AS IT IS - the contract of
 * pychain_C.forward_backward_log_domain, whose C++ does not clamp (chain-log-domain-computation.cc:137-145; the reference
 * clamps in Python, pychain/loss.py:30).  Without it the host twin applies ChainFunction's clamp(-30, 30) itself. */
#define PYCHAIN_HIP_CPU_NO_CLAMP 0x100
size_t pychain_hip_num_workspace_bytes(int B, int T, int num_states, int num_transitions, int num_pdfs);
int pychain_hip_num_forward_backward(
    const int32_t* forward_transitions,         /* dev [G,K,3] */
    const int32_t* forward_transition_indices,  /* dev [G,H,2] */
    const float*   forward_transition_probs,    /* dev [G,K] log-probs */
    const int32_t* backward_transitions,        /* dev [G,K,3] */
    const int32_t* backward_transition_indices, /* dev [G,H,2] */
    const float*   backward_transition_probs,   /* dev [G,K] */
    const float*   initial_probs,               /* dev [G,H] log */
    const float*   final_probs,                 /* dev [G,H] log */
    int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions,
    int grad_mode, float grad_scale,
    float* objf_per_seq, float* grad /* fp32 whatever nnet_output_dtype */, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream);
/* 1 if the numerator's recursions read 2-byte network outputs for this shape (the tile kernels' float4-chunk forms; not the
 * general kernels, not option num_compat).  The gradient of pychain_hip_num_forward_backward stays fp32. */
int pychain_hip_num_half_native(int num_states, int num_transitions, int num_pdfs);

/* ------------------------------------------------------------------------
 * Viterbi forced alignment over log-domain numerator graphs (ABI 18): the best path through each sequence's graph.  Graphs,
 * graph_batch_stride, nnet_output (raw, clamped to [-30, 30] in-kernel) and the shapes as in pychain_hip_num_forward_backward;
 * only the backward-transition arrays (the arcs entering each state), initial_probs and final_probs are read.
 * Let x be the clamped input widened to fp64 and take the arcs entering h in the order of backward_transition_indices[h] = [lo, hi)
 * (columns src, dst, pdf; log-prob lp).  Then, in fp64 adds and compares only (no contraction, no transcendental):
 *   s(0,h)   = initial(h)
 *   s(t+1,h) = max over k in [lo,hi) of  s(t,src_k) + ((double)lp_k + x(t,pdf_k))     exactly this association;
 *              ties: the FIRST k in list order wins (a later arc replaces only on strictly greater); no arc: -inf
 *   score    = max over h of s(L,h) + (double)final(h)                                 ties: the lowest h
 * Outputs (dev; the host twin: host):
 *   score_per_seq[b]  double [B]: the best-path log-score, final weight included.  NaN (0x7ff8000000000000) if an arc of the
 *                     sequence's graph emits a NaN column of x at some frame t < L; -inf if no path of length L reaches a final state
 *   states[b][t]      int32 [B,T+1]: the state occupied before frame t, t = 0..L (states[b][L] = the final state); -1 beyond
 *   pdfs[b][t]        int64 [B,T]: the pdf of the arc taken from frame t to t+1; -1 for t >= L
 *   A sequence whose score is not finite has every row -1.  bad_count (dev int32[1]): sequences whose score is not finite,
 *   plus device-resident lengths outside [1, T] (the kernels clamp them).
 * The device and the host twin give the same bits.  Graphs the tile kernels take (pychain_hip_num_half_native's shapes) keep
 * uint16 backpointers (2 B T H bytes of workspace); larger ones run on a global-memory kernel with int32 backpointers.
 * 2-byte network outputs: pychain_hip_align_half_native says where the kernels read them as they are (else up-cast first).
 * nnet_output and the transition index tensors must be 16-byte aligned, else PYCHAIN_HIP_EINVAL (the device entry point; the
 * time windows of pychain_hip_align_tw are read one element at a time: any element-aligned start).
 * pychain_hip_cpu_align: fp32 input, host threads as the other host twins. */
size_t pychain_hip_align_workspace_bytes(int B, int T, int num_states, int num_transitions, int num_pdfs);
int pychain_hip_align(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions,
    double* score_per_seq, int32_t* states, int64_t* pdfs, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream);
int pychain_hip_align_half_native(int num_states, int num_transitions, int num_pdfs);
int pychain_hip_cpu_align(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions,
    double* score_per_seq, int32_t* states, int64_t* pdfs, int32_t* bad_count, int num_threads);

/* ------------------------------------------------------------------------
 * Alignment time windows on numerator graphs (ABI 19): constrained ("regular") LF-MMI, the numerator restricted to the paths
 * that stay near a given alignment.  The *_tw entry points are the entry points of the same name without the suffix, with one
 * argument more, last:
 *   time_windows  int32 [B][H][2] = {lo, hi} (dev; the host twin: host), H = num_states of the call.  One row per sequence,
 *                 also where the graph is shared (graph_batch_stride 0).  NULL = no windows: exactly the call without them.
 * State h is ADMISSIBLE at time index t in [0, L] iff lo <= t <= hi.  Any int32 values are legal: lo > hi = never,
 * lo <= 0 and hi >= L = always.  t is the index of alpha and of pychain_hip_align's states: "the state before frame t".
 * With adm(t,h) for admissible and x the clamped input as in pychain_hip_num_forward_backward:
 *   alpha(0,h) = initial(h)                                           if adm(0,h)   else -inf
 *   alpha(t,h) = LogSum_k alpha(t-1,src_k) + lp_k + x(t-1,pdf_k)      if adm(t,h)   else -inf     t = 1..L
 *   beta(L,h)  = final(h)                                             if adm(L,h)   else -inf
 *   beta(t,h)  = LogSum_k lp_k + beta(t+1,dst_k) + x(t,pdf_k)         if adm(t,h)   else -inf     t = L-1..0
 *   logP       = LogSum_h alpha(L,h) + final(h)
 * - the sum over the paths whose state lies in its window at every time.  Occupancies follow as without windows; they are
 * zero on every arc with an inadmissible end.  The mask is a select AFTER the log-sum: a masked state's value and its arcs'
 * log-shares are -inf whatever the sum was, so a NaN term that reaches only masked states goes no further (the host twin
 * does the same).  Windows that admit every state at every time give the same bits as NULL (objectives, gradient,
 * bad_count, totals).  A sequence whose windows admit no path gets logP = -inf and counts in bad_count, like a graph with no
 * path of length L.  Option num_compat = 1 (the reference's own arithmetic) takes no windows: such a call fails
 * (PYCHAIN_HIP_EUNSUPPORTED, pychain_hip_last_error says why).  The fused calls offset the windows with the sequences of a
 * slice; pychain_hip_chain_loss_backward reads the stored rows and takes none.  pychain_hip_align takes them as pychain_hip_align_tw
 * (ABI 26, below). */
int pychain_hip_num_forward_backward_tw(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions, int grad_mode, float grad_scale,
    float* objf_per_seq, float* grad, int32_t* bad_count, void* workspace, size_t workspace_bytes, void* stream,
    const int32_t* time_windows);
int pychain_hip_chain_loss_forward_tw(
    const void* plans_dev, int64_t plan_stride_bytes, int resident_slot_rows, int den_num_states, float leaky_hmm_coefficient,
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride, int num_num_states, int num_num_transitions,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    float* den_objf_per_seq, float* num_objf_per_seq, void* grad, float grad_scale, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_workspace, size_t den_workspace_bytes, void* num_workspace, size_t num_workspace_bytes, void* stream,
    const int32_t* time_windows);
int pychain_hip_chain_loss_forward_backward_tw(
    const void* plans_dev, int64_t plan_stride_bytes, int resident_slot_rows, int den_num_states, float leaky_hmm_coefficient,
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride, int num_num_states, int num_num_transitions,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs, float grad_scale,
    float* den_objf_per_seq, float* num_objf_per_seq, void* grad, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_workspace, size_t den_workspace_bytes, void* num_workspace, size_t num_workspace_bytes, void* stream,
    const int32_t* time_windows);
int pychain_hip_cpu_num_forward_backward_tw(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions, int grad_mode, float grad_scale,
    float* objf_per_seq, float* grad, int32_t* bad_count, int num_threads, const int32_t* time_windows);

/* ------------------------------------------------------------------------
 * Constrained re-alignment (ABI 26): pychain_hip_align under the time windows above - the best path among the paths that keep
 * every state inside its window.  pychain_hip_align_tw / pychain_hip_cpu_align_tw are pychain_hip_align / pychain_hip_cpu_align
 * with one argument more, last: time_windows, int32 [B][H][2] = {lo, hi} (dev; the host twin: host), one row per sequence also
 * where the graph is shared, adm(t,h) iff lo <= t <= hi for the time index t in [0, L] exactly as above.  With the arcs, x and
 * the arithmetic of pychain_hip_align (fp64 adds and compares only, its association, its tie rules):
 *   s(0,h)   = initial(h)                                                     if adm(0,h)   else -inf
 *   s(t+1,h) = max over k in [lo,hi) of  s(t,src_k) + ((double)lp_k + x(t,pdf_k))     if adm(t+1,h) else -inf
 *   score    = max over the h with adm(L,h) of  s(L,h) + (double)final(h)             ties: the lowest h
 * The mask is a select AFTER the max, and the NaN rule follows the numerator's ("a NaN term that reaches only masked states
 * goes no further"): an arc term counts towards the NaN score only if its destination is admissible at t+1, a final term only
 * if its state is admissible at L.  A sequence whose windows admit no path gets score -inf, every row -1 and one count in
 * bad_count, as a graph with no path of length L does.  time_windows NULL: exactly pychain_hip_align, which forwards NULL.
 * Windows that admit every state at every time (lo <= 0 and hi >= L; also -1 .. 2^31-1) give the same bits as NULL: score
 * words, states, pdfs and bad_count.  The device and the host twin give the same bits.  The workspace is that of
 * pychain_hip_align (pychain_hip_align_workspace_bytes); the windows are read where they are. */
int pychain_hip_align_tw(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions,
    double* score_per_seq, int32_t* states, int64_t* pdfs, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream, const int32_t* time_windows);
int pychain_hip_cpu_align_tw(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions,
    double* score_per_seq, int32_t* states, int64_t* pdfs, int32_t* bad_count, int num_threads, const int32_t* time_windows);

/* ------------------------------------------------------------------------
 * Numerator posteriors as cross-entropy targets (ABI 20): the "xent regularisation" of chain training.  A second output of the
 * network, z [B,T,D] (raw, NOT clamped; its own dtype), is trained by cross-entropy against the numerator occupancies of the same
 * call.  With gamma_b(t,d) the numerator occupancy of the call (under its time windows, if any) and s_b(t) = sum_d gamma_b(t,d):
 *   xent_objf[b]       = sum_{t < L_b} ( sum_d gamma_b(t,d) z(t,d)  -  s_b(t) logsumexp_d z(t,.) )
 *   d xent / d z(b,t,d) = gamma_b(t,d) - s_b(t) softmax(z(t,.))_d        for t < L_b, exactly 0 for t >= L_b
 * gamma is a constant target: nothing flows back to the chain output through it (Kaldi copies the numerator posteriors and does
 * not differentiate them).  A sequence whose logP is not finite (no admissible path) has gamma = 0: objective 0, zero gradient
 * rows.  The row of z is read once; maximum, sum and the row itself stay on chip in fp32 between the reduction and the store
 * (exp and log in fp32); terms with gamma = 0 are left out of the dot product.  A NaN or an infinity in a live row of z makes that
 * sequence's xent objective what torch.log_softmax would make it (NaN); the LF-MMI objectives, the LF-MMI gradient and bad_count do
 * not see z at all.  Frame objectives are added up per sequence in fp64 in a fixed order: the same call gives the same bits.
 *
 * The *_xent entry points are the *_tw entry points of the same name with one argument more, last: a pointer to the struct below
 * (host memory, read during the call only).  NULL = exactly the call without it: same launches, same bits.
 *   z, z_dtype         dev [B,T,D] (the host twin: host, fp32 only), PYCHAIN_HIP_F32 / _BF16 / _F16; 2-byte rows are read as they are
 *   xent_grad          dev [B,T,D] in z_dtype, or NULL (no store: z needs no gradient).  Every element is written ONCE:
 *                      xent_grad = grad_scale [* *grad_scale_dev] [/ *loss_norm_dev] * (gamma - s softmax(z)), rounded at the store;
 *                      rows t >= L_b are zeros.  A trainer passes grad_scale = -c * upstream [/ frames].
 *   xent_objf_per_seq  dev float [B]
 *   xent_totals        dev float [2] or NULL: [0] = loss_scale * S [/ *loss_norm_dev] with S = sum_b xent_objf[b] (fp64, fixed order;
 *                      loss_scale, loss_norm_dev: those of a fused call, 1 and none elsewhere), [1] = S
 *   loss_coef          fused calls with `totals`: totals[0] and totals[4] become the full loss, LF-MMI + loss_coef * xent_totals[0]
 *                      (a trainer passes -c); totals[1..3], totals[5..7] keep their meaning and their bits
 *   workspace          dev, pychain_hip_xent_workspace_bytes(B, T, num_states, num_transitions, num_pdfs) bytes, 16-byte aligned:
 *                      the frame objectives (8 B T bytes) and, for numerator graphs on the general kernels - which leave no compact
 *                      occupancy rows - a dense fp32 [B,T,D] posterior buffer (slow but complete, like every general path).  The
 *                      workspaces of the call itself are as large as without xent.  (The host twin takes none.)
 * pychain_hip_num_forward_backward_xent: `grad` may be NULL when xent is given (only the cross-entropy is wanted: the dense
 * occupancy pass is left out).  The fused calls run the row kernel on the numerator's side stream, behind the compact occupancy
 * launch and behind the event the denominator's occupancy launch waits for, and join it to `stream` before they return;
 * pychain_hip_chain_loss_forward without `grad` then runs the compact occupancy launch in forward as well.  A call in slices
 * (pychain_hip_chain_loss_slices) runs it slice by slice.  Option num_compat = 1 takes no xent: PYCHAIN_HIP_EUNSUPPORTED. */
typedef struct pychain_hip_xent {
  const void*  z;
  int          z_dtype;
  void*        xent_grad;
  float        grad_scale;
  const float* grad_scale_dev;
  float        loss_coef;
  float*       xent_objf_per_seq;
  float*       xent_totals;
  void*        workspace;
  size_t       workspace_bytes;
} pychain_hip_xent;
size_t pychain_hip_xent_workspace_bytes(int B, int T, int num_states, int num_transitions, int num_pdfs);
int pychain_hip_num_forward_backward_xent(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions, int grad_mode, float grad_scale,
    float* objf_per_seq, float* grad, int32_t* bad_count, void* workspace, size_t workspace_bytes, void* stream,
    const int32_t* time_windows, const pychain_hip_xent* xent);
int pychain_hip_chain_loss_forward_xent(
    const void* plans_dev, int64_t plan_stride_bytes, int resident_slot_rows, int den_num_states, float leaky_hmm_coefficient,
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride, int num_num_states, int num_num_transitions,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    float* den_objf_per_seq, float* num_objf_per_seq, void* grad, float grad_scale, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_workspace, size_t den_workspace_bytes, void* num_workspace, size_t num_workspace_bytes, void* stream,
    const int32_t* time_windows, const pychain_hip_xent* xent);
int pychain_hip_chain_loss_forward_backward_xent(
    const void* plans_dev, int64_t plan_stride_bytes, int resident_slot_rows, int den_num_states, float leaky_hmm_coefficient,
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride, int num_num_states, int num_num_transitions,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs, float grad_scale,
    float* den_objf_per_seq, float* num_objf_per_seq, void* grad, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_workspace, size_t den_workspace_bytes, void* num_workspace, size_t num_workspace_bytes, void* stream,
    const int32_t* time_windows, const pychain_hip_xent* xent);
/* the host twin: fp64 accumulation (occupancies, log-sum-exp, objective), host threads as the other twins */
int pychain_hip_cpu_num_forward_backward_xent(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions, int grad_mode, float grad_scale,
    float* objf_per_seq, float* grad, int32_t* bad_count, int num_threads, const int32_t* time_windows,
    const pychain_hip_xent* xent);

/* ------------------------------------------------------------------------
 * Output regularisers (ABI 21): the two element-wise terms of the chain objective over the network output x [B,T,D] itself,
 * Kaldi's --chain.l2-regularize and --chain.out-of-range-regularize (PenalizeOutOfRange).  With e(x) = max(|x| - limit, 0) on the
 * RAW x (limit = 30 is the kernels' own clamp: beyond it the LF-MMI objective is flat and its gradient is the occupancy whatever
 * x was - the penalty is what pulls such an output back),
 *   R2_b = sum_{t < L_b} sum_d x(b,t,d)^2          RO_b = sum_{t < L_b} sum_d e(x(b,t,d))^2
 *   term(x) = l2 * x + 2 * oor * sign(x) * e(x)    = d (0.5 * l2 * x^2 + oor * e(x)^2) / dx
 * One streaming pass over the live rows (t < L_b) only; rows t >= L_b are NEVER READ (a NaN in padding is harmless).  `grad`:
 *   NULL                      the objective only: x is read once, nothing else of [B,T,D] size is touched
 *   PYCHAIN_HIP_GRAD_ACCUM    grad(b,t,d) += s * term(x(b,t,d)) for t < L_b: the stored row is read once and written once, in the
 *                             gradient's dtype; rows t >= L_b are NOT TOUCHED
 *   PYCHAIN_HIP_GRAD_LINEAR   grad(b,t,d)  = s * term(x(b,t,d)) for t < L_b, zeros for t >= L_b: every element written once
 * with s = grad_scale [* *grad_scale_dev] [/ *loss_norm_dev], both scalars read on the device (no host sync).  `grad` has
 * nnet_output's dtype.  The gradient term is plain fp32 (csrc/outreg.hip writes its operation sequence down: 7 roundings at
 * most, the add into the stored gradient included).  A 2-BYTE GRADIENT IN ACCUM IS ROUNDED TWICE: the call that stored it rounded
 * it to bf16 / fp16, and this pass rounds the sum again.  Squares and sums are fp64 from the first add (x is widened first, so
 * x^2 and |x| - limit are exact), added up in a fixed order - lanes, then one {R2, RO} pair per frame, then the frames of a
 * sequence -, without float atomics: the same call gives the same bits.  A NaN or an infinity in a live row makes that
 * sequence's R2_b / RO_b what the torch composition would make them, and leaves the other sequences' values alone.
 *   reg_per_seq  dev float [B][2] = {R2_b, RO_b}, the fp64 sums rounded once
 *   reg_totals   dev float [3] or NULL: [0] = loss_scale * (0.5 l2 sum_b R2_b + oor sum_b RO_b) [/ *loss_norm_dev],
 *                [1] = sum_b R2_b, [2] = sum_b RO_b (fp64 over the unrounded per-sequence sums, rounded once)
 *   totals       dev float [PYCHAIN_HIP_TOTALS] or NULL: the totals of a fused call on the same stream.  The call's last kernel
 *                adds reg_totals[0] to totals[0] and totals[4] - one thread, in stream order behind the fused call and behind its
 *                xent totals - so they hold the full loss; totals[1..3] and totals[5..7] keep their bits.
 *   workspace    dev, pychain_hip_output_reg_workspace_bytes(B, T) bytes, 16-byte aligned: the frame pairs (fp64 [B,T,2]) and the
 *                unrounded per-sequence sums
 * Lengths outside [1,T] are clamped, as everywhere.  Any D >= 1: 16-byte loads and stores where the rows allow (fp32 rows of a
 * multiple of 4 elements, 2-byte rows of a multiple of 8; 8-byte ones for 2-byte rows of a multiple of 4), else element by
 * element.  l2 < 0, oor < 0, limit < 0 or a grad_mode other than the two above: PYCHAIN_HIP_EINVAL.  nnet_output, grad and
 * workspace must be 16-byte aligned.  The entry point is a translation unit of its own: the objects of den_*.hip, num_*.hip,
 * xent.hip and align.hip do not change, and no existing entry point launches anything it did not launch before. */
size_t pychain_hip_output_reg_workspace_bytes(int B, int T);
int pychain_hip_output_reg(
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    float l2, float oor, float limit, int grad_mode, void* grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    float* reg_per_seq, float loss_scale, float* reg_totals, float* totals,
    void* workspace, size_t workspace_bytes, void* stream);
/* the host twin: the same on host pointers (the two scalars too), fp32 rows, the same fp32 operation sequence of the gradient term
 * and fp64 sums; no workspace, no stream */
int pychain_hip_cpu_output_reg(
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    float l2, float oor, float limit, int grad_mode, float* grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    float* reg_per_seq, float loss_scale, float* reg_totals, float* totals, int num_threads);

/* ------------------------------------------------------------------------
 * Utterance weights and per-frame derivative weights (ABI 22): the two pieces of Kaldi's chain objective that come with a
 * minibatch - Supervision::weight (u, float [B]) and NnetChainSupervision::deriv_weights (f, float [B,T], --apply-deriv-weights) -
 * applied behind a call that has left a gradient and its per-sequence objectives on the device.  A missing factor (NULL) is 1;
 * both NULL: PYCHAIN_HIP_EINVAL (there is nothing to do, and a caller without weights never comes here).
 * ROWS (`grad` dev [B,T,D] of grad_dtype, or NULL: the sums only), in place, one streaming pass over the live rows; per
 * (b, t < L_b), w = fl32(u_b * f_bt):
 *   w == 1   the row is NEITHER READ NOR WRITTEN
 *   w == 0   the row is stored as +0 WITHOUT A LOAD (a NaN or an infinity in it is gone)
 *   else     every element is widened to fp32 (exact), multiplied ONCE by w and rounded ONCE, to nearest even, to grad_dtype:
 *            grad(b,t,d) = round(fl32(w * grad(b,t,d))) - one IEEE multiply, one rounding, the same bits on every run
 * Rows t >= L_b are NEVER TOUCHED.  The pass moves the bytes of the rows it changes: derivative weights that are 1 except at the
 * edges of a chunk cost those edge rows.  Any D >= 1: 16-byte accesses where the rows allow (fp32 rows of a multiple of 4
 * elements, 2-byte rows of a multiple of 8; 8-byte ones for 2-byte rows of a multiple of 4), else element by element.  Weights
 * are not inspected: a negative or non-finite one is multiplied in as it is.  f scales derivative rows ONLY - neither the
 * objective nor its normaliser, as in Kaldi - so with f the gradient is deliberately not the gradient of the scalar.
 * SUMS (`totals` or `weighted` given; den_objf_per_seq and num_objf_per_seq are then required): over the per-sequence arrays
 * a fused call leaves,
 *   term_b = den_b - num_b [+ xent_coef * xent_b] [+ 0.5 * l2 * R2_b + oor * RO_b]     (reg_per_seq = {R2_b, RO_b} [B][2]; a
 *                                                                                       trainer passes xent_coef = -c)
 * in fp64, ascending b on one thread, no float atomics, each result rounded once.  AN UTTERANCE WITH u_b == 0 IS SKIPPED, not
 * multiplied: its objective may be -inf or a NaN and contributes exactly 0 to every sum.
 *   totals    dev float [PYCHAIN_HIP_TOTALS] or NULL, the totals of the fused call on the same stream (behind its xent totals and
 *             behind pychain_hip_output_reg): totals[0] = totals[4] = loss_scale * sum_b u_b term_b [/ *loss_norm_dev],
 *             totals[1] = sum_b u_b L_b (the normaliser of an averaged loss: what a sharded trainer all-reduces),
 *             totals[3] = sum_b u_b (den_b - num_b); totals[2] and totals[5..7] keep their bits.
 *   weighted  dev float [5] or NULL: {sum u (den - num), sum u xent, sum u R2, sum u RO, sum u L}
 * The caller passes the loss_norm_dev (or folds 1 / sum_b u_b L_b into the scales) it gave the fused call: the gradient that
 * call wrote is already divided by it.  Lengths outside [1,T] are clamped, as everywhere.  grad must be 16-byte aligned.  The
 * entry point is a translation unit of its own (csrc/weights.hip): the objects of den_*.hip, num_*.hip, xent.hip, align.hip
 * and outreg.hip do not change, and no existing entry point launches anything it did not launch before. */
int pychain_hip_weight_rows(
    void* grad, int grad_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const float* utt_weights, const float* deriv_weights,
    const float* den_objf_per_seq, const float* num_objf_per_seq, const float* xent_objf_per_seq, float xent_coef,
    const float* reg_per_seq, float l2, float oor, float loss_scale, const float* loss_norm_dev,
    float* totals, float* weighted, void* stream);
/* the host twin: the same on host pointers, fp32 rows, the same single multiply and the same fp64 sums; no stream */
int pychain_hip_cpu_weight_rows(
    float* grad, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const float* utt_weights, const float* deriv_weights,
    const float* den_objf_per_seq, const float* num_objf_per_seq, const float* xent_objf_per_seq, float xent_coef,
    const float* reg_per_seq, float l2, float oor, float loss_scale, const float* loss_norm_dev,
    float* totals, float* weighted, int num_threads);

/* ------------------------------------------------------------------------
 * Posterior-target supervision (ABI 23): the numerator of the chain objective as sparse per-frame posterior targets instead of a
 * graph - q(b,t,k) on the pdfs pdf(b,t,k), K entries per frame, from a teacher model or from lattice posteriors of unlabelled
 * audio (Kaldi: the "KL" objective of teacher-student and semi-supervised chain training).  The objective is
 * sum q x - log Z_den, its derivative q - gamma_den.  C callers: call pychain_hip_den_forward_backward, then
 * pychain_hip_post_targets on the same stream, with the gradient, the per-sequence objectives and the totals the first left.
 * ENTRIES.  (b,t,k) is live when t < L_b and 0 <= pdf < D.  pdf < 0 is padding and is skipped; pdf >= D in a live frame is
 * skipped and counted in bad_count (dev int32[1], written by the call).  Rows and entries with t >= L_b are NEVER READ (a NaN in
 * them is harmless).  Lengths outside [1,T] are clamped, as everywhere.  Targets need not sum to 1 per frame: they are
 * multiplied in as given.
 * OBJECTIVE.  num_objf_per_seq[b] = sum_{t < L_b} sum_k q_k * clamp(x(b,t,pdf_k), -30, 30).  x and q are widened to fp64 first,
 * so every product is exact; the sum is fp64 in a fixed order - k within a frame, one value per frame into the workspace, then
 * the frames of a sequence -, without float atomics, rounded once: the same call gives the same bits.  A NaN in a referenced live
 * element makes that sequence's objective a NaN and leaves the other sequences' objectives alone.
 * GRADIENT (`grad` dev [B,T,D] of nnet_output's dtype, or NULL: the objective only).  For every live frame and every distinct
 * pdf d in it, qd = the fp32 sum of the frame's q_k with pdf_k == d, in ascending k, and
 *   grad(b,t,d) = round(fmaf(s, qd, (float)grad(b,t,d)))         ONE fma, one rounding to the gradient's dtype
 * with s = grad_scale [* *grad_scale_dev] [/ *loss_norm_dev], both scalars read on the device, formed in fp32 as
 * pychain_hip_output_reg forms it.  ONLY THE ADDRESSED ELEMENTS ARE TOUCHED.  The clamp is not differentiated, as in the rest of
 * the library.  A trainer passes s < 0 behind a denominator call that wrote grad_scale * gamma_den (the convention of
 * PYCHAIN_HIP_GRAD_ACCUM).  A 2-BYTE GRADIENT IS THEREBY ROUNDED TWICE: the call that stored it rounded it to bf16 / fp16, and
 * this pass rounds the sum again.  One thread owns a frame: a pdf that occurs several times in it does not race.
 * TOTALS (`totals` dev float [PYCHAIN_HIP_TOTALS] or NULL: the totals of the denominator call on the same stream;
 * den_objf_per_seq, dev [B], is then required).  One thread, in stream order behind that call, in ascending b and in fp64 over
 * the float denominator objectives and the unrounded numerator sums:
 *   totals[3] = S = sum_b den_b - sum_b num_b,   totals[0] = totals[4] = loss_scale * S [/ *loss_norm_dev],
 *   totals[2] += the bad entries;   totals[1] and totals[5..7] keep their bits
 * - the layout a fused call leaves, so pychain_hip_output_reg and pychain_hip_weight_rows work behind this call unchanged.
 *   workspace   dev, pychain_hip_post_targets_workspace_bytes(B, T) bytes, 16-byte aligned
 * Any K >= 1 and any D >= 1.  K < 1, a NULL required pointer, or a grad or workspace that is not 16-byte aligned:
 * PYCHAIN_HIP_EINVAL.  The entry point is a translation unit of its own (csrc/post.hip): the objects of den_*.hip, num_*.hip,
 * xent.hip, align.hip, outreg.hip and weights.hip do not change, and no existing entry point launches anything it did not
 * launch before. */
size_t pychain_hip_post_targets_workspace_bytes(int B, int T);
int pychain_hip_post_targets(
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, void* grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    const float* den_objf_per_seq, float* num_objf_per_seq, int32_t* bad_count,
    float loss_scale, float* totals, void* workspace, size_t workspace_bytes, void* stream);
/* the host twin: the same on host pointers (the two scalars too), fp32 rows, the same fma - its fp32 gradient has the device's
 * bits - and the same fp64 sums; no workspace, no stream */
int pychain_hip_cpu_post_targets(
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, float* grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    const float* den_objf_per_seq, float* num_objf_per_seq, int32_t* bad_count,
    float loss_scale, float* totals, int num_threads);
/* Sparse targets out of dense posterior rows (the teacher side).  Per live frame the elements of rows(b,t,:) are ordered by
 * value descending, index ascending; a NaN never wins a comparison and is never selected.  The first K elements with
 * value >= floor fill the slots in that order; unfilled slots get pdf = -1, prob = 0.  Values are the inputs widened to fp32
 * (exact); with `normalize` each is divided by the fp32 sum of the selected values taken in slot order (IEEE division).  A frame
 * with nothing selected stays all -1 / 0.  Frames t >= L_b are WRITTEN -1 / 0 and their rows never read.  out_pdfs int32
 * [B,T,K], out_probs float [B,T,K].  1 <= K <= min(num_pdfs, 64), else PYCHAIN_HIP_EINVAL.  Rows of up to 9216 elements are
 * read from memory once and held on chip; longer rows are re-read.  `rows` may start at any element-aligned address: 16-byte
 * loads where it starts on the 16-byte grid and num_pdfs is a multiple of the load's width, else one element at a time - the
 * selection is exact either way, and the outputs do not depend on which (tests/test_gpu_layouts.py holds them to the bit). */
int pychain_hip_topk_rows(const void* rows, int rows_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
                          int K, float floor, int normalize, int32_t* out_pdfs, float* out_probs, void* stream);
int pychain_hip_cpu_topk_rows(const float* rows, const int64_t* seq_lengths, int B, int T, int num_pdfs,
                              int K, float floor, int normalize, int32_t* out_pdfs, float* out_probs, int num_threads);

/* ------------------------------------------------------------------------
 * Cross-entropy against sparse targets (ABI 24): the xent term of chain training where the supervision is posterior targets (the
 * teacher-student and semi-supervised recipes train their xent output against the same posteriors), and frame cross-entropy
 * against an alignment (hard targets, K = 1).  z is a network output [B,T,D], RAW (not clamped), fp32 / bf16 / fp16; the
 * targets are pdf(b,t,k) int32 and q(b,t,k) float, both [B,T,K], any K >= 1; lengths outside [1,T] are clamped, as everywhere.
 * ENTRIES.  (b,t,k) is live when t < L_b and 0 <= pdf < D.  pdf < 0 is padding and is skipped; pdf >= D in a live frame is
 * skipped and counted in bad_count (dev int32[1], written by the call).  Nothing with t >= L_b is ever read - neither entries
 * nor rows of z: a NaN there is harmless.
 * PER FRAME.  For every distinct pdf d of a frame, qd = the fp32 sum of the frame's q_k with pdf_k == d, in ascending k (the
 * rule of pychain_hip_post_targets: a repeated pdf is handled where it occurs first, nothing races, nothing is atomic);
 * s(t) = sum_d qd (targets need not sum to 1), and
 *   objective(b,t) = sum_d qd z(t,d) - s(t) logsumexp_d z(t,.)          d / dz(b,t,d) = qd - s(t) softmax(z(t,.))_d
 * Maximum, exp and log in fp32; the frame value is (double)dot - (double)s * (double)lse; the frames of a sequence are added in
 * fp64 in a fixed order and rounded once into xent_objf_per_seq[b] (dev float [B]).  A LIVE FRAME WITHOUT A LIVE ENTRY has
 * objective 0, its gradient row is stored as zeros and ITS ROW OF z IS NOT READ: sparse supervision costs the frames it
 * supervises.  A NaN or an infinity in a row that is read does what log_softmax does: that sequence's objective is a NaN, the
 * others are untouched.
 * GRADIENT (`xent_grad` dev [B,T,D] in z's dtype, or NULL: the form without the store).  Every element is written ONCE:
 *   grad_scale [* *grad_scale_dev] [/ *loss_norm_dev] * (qd - s softmax),   rounded at the store;   rows t >= L_b: zeros
 * 2-byte rows are read as they are; the values, and the gradient before its rounding, are the bits of the same call on the
 * up-cast fp32 z.  No float atomics: the same call gives the same bits.  Rows of more than 24 576 pdfs do not fit LDS and are
 * re-read from memory by every pass (slow but complete).
 *   workspace   dev, pychain_hip_xent_targets_workspace_bytes(B, T) bytes, 16-byte aligned
 * K < 1, a NULL required pointer, or a z, xent_grad or workspace that is not 16-byte aligned: PYCHAIN_HIP_EINVAL.  The call runs
 * the rows, the per-sequence sums and the bad count on `stream`; it depends on nothing else of a training step. */
size_t pychain_hip_xent_targets_workspace_bytes(int B, int T);
int pychain_hip_xent_targets(
    const void* z, int z_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, void* xent_grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    float* xent_objf_per_seq, int32_t* bad_count, void* workspace, size_t workspace_bytes, void* stream);
/* The totals step behind it (what the *_xent entry points do for their own term): with S = sum_b xent_objf_per_seq[b] in fp64,
 *   xent_totals[0] = loss_scale * S [/ *loss_norm_dev],   xent_totals[1] = S             (dev float[2], or NULL)
 *   totals[0] = totals[4] = totals[0] + loss_coef * xent_totals[0],   totals[2] += *bad_count      (dev float[8], or NULL)
 * - the other words of `totals` keep their bits; `bad_count` (dev int32[1]) may be NULL.  One small launch, in stream order
 * behind whatever wrote `totals`. */
int pychain_hip_xent_add_totals(const float* xent_objf_per_seq, int B, float loss_scale, const float* loss_norm_dev, float loss_coef,
                                float* xent_totals, float* totals, const int32_t* bad_count, void* stream);
/* the host twin: the same on host pointers (the two scalars too), fp32 z, qd by the same fp32 rule, fp64 log-sum-exp and sums,
 * host threads over the sequences; zeros beyond a length; no workspace, no stream */
int pychain_hip_cpu_xent_targets(
    const float* z, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, float* xent_grad,
    float grad_scale, const float* grad_scale_dev, const float* loss_norm_dev,
    float* xent_objf_per_seq, int32_t* bad_count, int num_threads);

/* ------------------------------------------------------------------------
 * Boosted denominator rows (ABI 25): the margin of the boosted objective (LF-bMMI).  The denominator is evaluated with every
 * path's score lowered by `boost` times its per-frame agreement with a reference a(b,t,n), given as sparse per-frame targets
 * (the layout and the index type of pychain_hip_post_targets: an alignment as K = 1 hard targets, or posterior targets):
 *   F = num(x) - log sum_paths p(path) prod_t exp(clamp(x(t, pdf_t), -30, 30) - boost * a(t, pdf_t))
 * - bMMI up to the path-independent constant boost * T, which is dropped; THE MARGIN IS APPLIED BEHIND THE CLAMP, so it does not
 * vanish where |x| is near 30.  This call writes the rows the denominator then reads as they are: C callers run
 * pychain_hip_boost_rows, then pychain_hip_den_forward_backward(e, PYCHAIN_HIP_F32, input_is_exp = 1) on the same stream; the
 * occupancies that call writes are the boosted denominator's gradient with respect to x (neither the clamp nor the reference is
 * differentiated).  For every live frame (b, t < L_b):
 *   e(b,t,n) = E = exp(clamp(x(b,t,n)))       every n: the clamp and the exp of the denominator kernels themselves (v_med3_f32, then
 *                                             v_exp_f32 on the rounded product with fp32(log2 e)) - an element no entry addresses
 *                                             has the bits the denominator would have formed from x
 *   e(b,t,d) = fl32(E * F)                    every distinct pdf d of the frame's live entries; qd = the fp32 sum, in ascending k, of
 *                                             the frame's q_k with pdf_k == d (handled where d occurs first: a repeated pdf is
 *                                             applied once, nothing races, nothing is atomic), u = fl32(boost * qd),
 *                                             F = v_exp_f32(fl32(-u * fp32(log2 e))): two roundings and the hardware exp2 make
 *                                             F, ONE multiply makes e
 * ENTRIES.  pdf < 0 is padding and is skipped; pdf >= D in a live frame is skipped and counted.  Rows of x, rows of e and entries
 * with t >= L_b are NEITHER READ NOR WRITTEN.  Lengths outside [1,T] are clamped, as everywhere.  A NaN in a live row of x becomes
 * exp(-30) (the clamp's v_med3_f32) and would reach no check of the denominator call behind, so it is counted here:
 *   bad_count  dev int32[1], written by the call: the live entries with pdf >= D + the live frames of x that hold a NaN
 * One streaming pass: x read once in its own type (fp32 / bf16 / fp16, any D; 16-byte accesses of the fp32 side where D is a
 * multiple of 4), e written once in fp32.  boost must be finite and >= 0 (0: e = E everywhere); K >= 1; nnet_output and e 16-byte
 * aligned; else PYCHAIN_HIP_EINVAL.  The entry point is a translation unit of its own (csrc/boost.hip): no other object changes,
 * and no existing entry point launches anything it did not launch before. */
int pychain_hip_boost_rows(
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, float boost,
    float* e, int32_t* bad_count, void* stream);
/* the host twin: the same on host pointers, fp32 rows, the same operation sequence with exp2f of the host's libm where the device
 * has v_exp_f32 - its e has the device's bits wherever the two exp2 agree, and is within the two roundings and the two exp2
 * errors otherwise; host threads over the sequences; no stream */
int pychain_hip_cpu_boost_rows(
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, float boost,
    float* e, int32_t* bad_count, int num_threads);

/* ------------------------------------------------------------------------
 * Lattice-free sMBR (ABI 27): the expected frame accuracy of the denominator's path distribution against a reference, and its
 * gradient (state-level minimum Bayes risk without lattices; Kanda et al., Interspeech 2018).  The reference is
 * sparse per-frame targets (the layout and the index type of pychain_hip_post_targets: an alignment as K = 1 hard targets, or
 * posterior targets); the accuracy of pdf n at frame t is A(t,n) = the sum of the frame's q_k with pdf_k == n (repeated pdfs
 * add, padding adds nothing).  A path scores sum_t A(t, pdf of its arc at t); leak transitions score nothing.  Per sequence:
 *   E          = sum_paths P(path) score(path) = sum_t e(t),   e(t) = sum_n gamma(t,n) A(t,n)
 *   dE/dy(t,n) = gamma(t,n) (E[score | pdf n at t] - E)                       y the network output, x = exp(clamp(y, -30, 30))
 * with gamma the denominator's occupancies under the leaky-HMM model of pychain_hip_den_forward_backward.  Neither the clamp nor
 * the reference is differentiated.  Every live row of the gradient sums to zero over n.
 *
 * THE CALL HAS TWO STAGES, on one stream:
 *   1. pychain_hip_den_forward_backward(x, ..., grad_scale = 1) as it is: its gradient IS gamma, [B,T,D] fp32 (a 2-byte network
 *      output is up-cast for this stage).  pychain_hip_smbr_frame_accuracy then forms e(b,t) and E_b = sum_t e(b,t) (fp64).
 *   2. pychain_hip_smbr_forward_backward: the gradient is a covariance under the path distribution and needs, beside alpha' and
 *      beta', an accuracy-weighted pair of recursions (v' = the leak of v, the same operator for both of a pair):
 *        abar(0) = 0   abar(t+1,j) = sum_{k: dst=j} [ abar'(t,src) + a(t,pdf_k) alpha'(t,src) ] p_k x(t,pdf_k)
 *        bbar(L) = 0   bbar(t,i)   = sum_{k: src=i} p_k x(t,pdf_k) [ bbar'(t+1,dst) + a(t,pdf_k) beta'(t+1,dst) ]
 *        q0(t,n) = sum_{k: pdf=n} p alpha'(t,src) beta'(t+1,dst)
 *        q1(t,n) = sum_{k: pdf=n} p [ abar'(t,src) beta'(t+1,dst) + alpha'(t,src) bbar'(t+1,dst) ]
 *        v(t,n) = x(t,n) (q1(t,n) + a(t,n) q0(t,n))        eps(t) = sum_m v(t,m) / sum_m x(t,m) q0(t,m)
 *        grad(t,n) = s (v(t,n) - eps(t) x(t,n) q0(t,n)) / sum_m x(t,m) q0(t,m)           s = grad_scale [* *grad_scale_dev]
 *      with the CENTRED accuracies a(t,n) = A(t,n) - e(t): a per-frame constant changes no covariance, and it keeps the weighted
 *      quantities from growing like t.  eps is zero in exact arithmetic.  In fp32 it is the rounding of e(t), which every frame
 *      leaves in abar and bbar and the recursions carry on: every live row is centred by its own mean, or it would carry
 *      gamma(t,n) times the residue accumulated over the whole sequence.  All four vectors are normalised
 *      per frame by the totals of alpha and beta; the quotient removes the factors.  One recursion launch of 2B persistent
 *      workgroups (sequence x direction; no workgroup waits for another), one time-parallel gradient launch.
 *
 * GRAPH.  One denominator graph for every sequence, in the reference layout as device pointers (fstext.cc:49-116): arcs
 * {src, dst, pdf} in runs by source (forward_*) and by destination (backward_*), [H,2] run bounds, probabilities, and the leaky,
 * initial and final probabilities [H]; every src, dst < H and pdf < num_pdfs (NOT checked: device memory).  pdf_arcs int32[K]:
 * the ids of the forward_* arcs ordered by pdf, stable; pdf_index int32[num_pdfs + 1]: the run of pdf n is
 * pdf_arcs[pdf_index[n] .. pdf_index[n+1]).
 * frame_accuracy:    gamma dev fp32 [B,T,D]; frame_acc dev float[B,T] out (live frames only); acc_per_seq dev double[B] out;
 *                    bad_count dev int32[2], ZEROED by this call: [1] = the live entries with pdf >= num_pdfs (skipped
 *                    otherwise; pdf < 0 is padding).  Frames t >= L_b are neither read nor written.
 * forward_backward:  nnet_output in its own type (fp32 / bf16 / fp16, read element by element: any element-aligned start);
 *                    frame_acc, acc_per_seq, bad_count as the first call left them; grad dev [B,T,D] out in the network output's
 *                    type, written once: rows t >= L_b are exact zeros, a pdf no arc carries gets an exact zero without its x
 *                    being read.  The 2-byte forms compute what the fp32 form computes on the up-cast input and round once.
 *                    closing dev float[B] out: sum_j abar'(L,j) final(j) / sum_j alpha'(L,j) final(j), a diagnostic of the
 *                    recursions: zero in exact arithmetic, in fp32 the UNCENTRED residue of e(t)'s rounding summed over the
 *                    sequence - it grows with the length (1e-6 at 1500 frames, 2e-3 from the host twin) and bounds nothing.  bad_count[0] += the sequences with a frame total of the recursions or a
 *                    frame's divisor sum_m x q0 of the gradient that is not positive and finite, or a NaN in a live row of x:
 *                    such a sequence has acc_per_seq NaN and is counted once; closing is NaN where the recursions or x were
 *                    the cause.  The other sequences of the call are untouched.
 * No float atomics: a call gives the same bits every time.  The recursion workgroup keeps four state vectors and four rows in
 * LDS: (4 H + 4 num_pdfs + 128) * 4 bytes must fit the 160 KiB of a CU (3000 states and 3456 pdfs: 103 KiB), else
 * PYCHAIN_HIP_EUNSUPPORTED with the sizes in the message - these two entry points have no slower form; the general kernels are
 * asked for by name (pychain_hip_smbr_forward_backward_general, below).  Workspace: pychain_hip_smbr_workspace_bytes
 * (the four trajectories, 16 (T + 1) H B bytes, and the frame totals).  leaky_hmm_coefficient in (0,1); K >= 1.  The entry points
 * are a translation unit of their own (csrc/smbr.hip): no existing entry point launches anything it did not launch before. */
size_t pychain_hip_smbr_workspace_bytes(int B, int T, int num_states);
int pychain_hip_smbr_frame_accuracy(
    const float* gamma, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K,
    float* frame_acc, double* acc_per_seq, int32_t* bad_count, void* stream);
int pychain_hip_smbr_forward_backward(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* leaky_probs, const float* initial_probs, const float* final_probs,
    const int32_t* pdf_arcs, const int32_t* pdf_index, int num_states, int num_transitions,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad /* nnet_output_dtype */, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream);
/* the host twins: the same equations on host pointers, fp32 rows, state vectors and gradient, fp64 sums; host threads over the
 * sequences; no workspace, no stream, any H and num_pdfs */
int pychain_hip_cpu_smbr_frame_accuracy(
    const float* gamma, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K,
    float* frame_acc, double* acc_per_seq, int32_t* bad_count, int num_threads);
int pychain_hip_cpu_smbr_forward_backward(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* leaky_probs, const float* initial_probs, const float* final_probs,
    const int32_t* pdf_arcs, const int32_t* pdf_index, int num_states, int num_transitions,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    float* grad, double* acc_per_seq, float* closing, int32_t* bad_count, int num_threads);

/* ------------------------------------------------------------------------
 * Lattice-free sMBR with the accuracy by CLASS (ABI 28): phone-level frame accuracy (Kaldi's --criterion=mpfe),
 * one class for all silence pdfs (--one-silence-class), or a reference that comes from another tree.  With a map
 * pdf_classes int32[num_pdfs] (device pointer; host pointer for the twins), every value in [0, num_classes) - NOT checked -
 *   Acls(t,c) = the sum, in ascending k, of the frame's q_k whose class is c       class_k = pdf_classes[id_k], or id_k itself
 *   A(t,n)    = Acls(t, pdf_classes[n])                                            when targets_are_classes
 * and everything else is the section above with this A: e(t), E, the centred a = A - e(t), the recursions, q0, q1, the gradient,
 * closing and the verdicts.  A row of A is dense now - every pdf of a class takes the credit - so these are kernels of their own
 * (csrc/smbr.hip: smbr_class_*); the pdf-level entry points launch what they launched.  The identity map gives the pdf-level
 * quantities (not their bits: the order of the sums differs); one class gives E_b = sum_t sum_k q_k and a zero gradient.
 * Padding (id < 0) adds nothing; an id that is out of range - >= num_pdfs for pdf targets, >= num_classes for class targets -
 * adds nothing and is counted in bad_count[1].
 *
 * Each entry point takes the arguments of its counterpart above, then pdf_classes, num_classes, targets_are_classes.
 * pdf_classes NULL is the call above, launch for launch and bit for bit (targets_are_classes must then be 0, num_classes is not
 * looked at); otherwise num_classes >= 1.
 * frame_accuracy_classes:   a dense pass over gamma, a wave per frame on a grid over (frames, B): 16-byte loads where num_pdfs is
 *                           a multiple of 4 and gamma and pdf_classes start on the 16-byte grid, else one element at a time; fp64
 *                           sums in a fixed order, no float atomics.  It takes a workspace behind the three
 *                           (pychain_hip_smbr_frame_accuracy_classes_workspace_bytes: the fp64 frame values E_b is summed from).
 * forward_backward_classes: the recursion workgroup keeps one table [num_classes] more in LDS, the gradient workgroup too:
 *                           pychain_hip_smbr_lds_bytes is what the larger of the two needs, static LDS included -
 *                           (4 H + 4 num_pdfs + num_classes + 128) * 4 bytes; num_classes = 0: the pdf-level form - and beyond the
 *                           160 KiB of a CU the call is refused, PYCHAIN_HIP_EUNSUPPORTED with H, num_pdfs, num_classes and both
 *                           byte counts in the message.  Workspace: pychain_hip_smbr_workspace_bytes, as above.
 * The properties of the pdf-level form hold: the same bits on every call; the 2-byte forms compute what the fp32 form computes on
 * the up-cast input and round once; a pdf no arc carries gets an exact zero, its x unread; rows t >= L_b are exact zeros. */
size_t pychain_hip_smbr_frame_accuracy_classes_workspace_bytes(int B, int T);
size_t pychain_hip_smbr_lds_bytes(int num_states, int num_pdfs, int num_classes);
int pychain_hip_smbr_frame_accuracy_classes(
    const float* gamma, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K,
    float* frame_acc, double* acc_per_seq, int32_t* bad_count, void* stream,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes,
    void* workspace, size_t workspace_bytes);
int pychain_hip_smbr_forward_backward_classes(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* leaky_probs, const float* initial_probs, const float* final_probs,
    const int32_t* pdf_arcs, const int32_t* pdf_index, int num_states, int num_transitions,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad /* nnet_output_dtype */, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes);
/* the host twins: the same equations on host pointers (pdf_classes too), no workspace */
int pychain_hip_cpu_smbr_frame_accuracy_classes(
    const float* gamma, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K,
    float* frame_acc, double* acc_per_seq, int32_t* bad_count, int num_threads,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes);
int pychain_hip_cpu_smbr_forward_backward_classes(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* leaky_probs, const float* initial_probs, const float* final_probs,
    const int32_t* pdf_arcs, const int32_t* pdf_index, int num_states, int num_transitions,
    const float* nnet_output, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    float* grad, double* acc_per_seq, float* closing, int32_t* bad_count, int num_threads,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes);

/* ------------------------------------------------------------------------
 * Lattice-free sMBR on graphs and trees beyond the LDS of a CU (ABI 29; csrc/smbr_general.hip).  The two
 * forward_backward entry points above keep four state vectors and four rows of a frame in LDS and refuse what does not fit:
 * 3000 states with more than about 7 200 pdfs (the 8408 pdfs of a 2000-frame tree among them), identity classes sooner, more
 * than about 10 000 states at any num_pdfs.  The general kernels take any num_states, num_pdfs, num_classes and K the int32
 * layout holds, with the same equations, row centring, checks and workspace layout; they are slower - what does not fit LDS is
 * gathered from global memory - and are asked for by name, through an entry point of their own:
 *   PYCHAIN_HIP_SMBR_LDS     the kernels of the entry points above, launch for launch
 *   PYCHAIN_HIP_SMBR_ROWS    the state vectors stay in LDS (pychain_hip_smbr_general_lds_bytes(num_states) within 160 KiB:
 *                            (4 H + 64) * 4 + 256 bytes); the frame's row x, its companion x A and the class table lie in
 *                            scratch rows of the workspace, one set per workgroup, made a frame ahead
 *   PYCHAIN_HIP_SMBR_GLOBAL  the state vectors too are read back from the trajectories in the workspace: always runs
 *   PYCHAIN_HIP_SMBR_AUTO    LDS where pychain_hip_smbr_lds_bytes is within 160 KiB, else ROWS where the state vectors fit, else
 *                            GLOBAL
 * The four codes name the forms of the expected arc counts too (pychain_hip_den_arc_counts_general, below): one set.
 * SAME BITS: thread-to-state and thread-to-pdf ownership, the arc order and the order of every sum are those of the LDS kernels,
 * so on a shape two forms take they give the same gradient, acc_per_seq, closing and bad_count, bit for bit.  No float atomics;
 * a call gives the same bits every time.
 * pychain_hip_smbr_form: host only; the form a call with `requested` would run, or PYCHAIN_HIP_EUNSUPPORTED (LDS or ROWS asked
 *   for on a shape it cannot hold: the sizes are in the message) or PYCHAIN_HIP_EINVAL (sizes, an unknown form).  num_classes 0:
 *   the pdf-level call.
 * pychain_hip_smbr_general_workspace_bytes: the trajectories of pychain_hip_smbr_workspace_bytes, then per recursion workgroup
 *   (2 B of them) 4 num_pdfs + num_classes floats and per gradient workgroup (at most 512, persistent over the (sequence, 8-frame
 *   block) items) 2 num_pdfs + num_classes floats, each rounded up to 256 bytes; 0 for bad sizes.  A call whose form resolves to
 *   LDS needs pychain_hip_smbr_workspace_bytes only.
 * pychain_hip_smbr_forward_backward_general: the arguments of pychain_hip_smbr_forward_backward_classes (pdf_classes NULL: the
 *   pdf-level call), then `form`; the same argument checks and messages. */
#define PYCHAIN_HIP_SMBR_AUTO   0
#define PYCHAIN_HIP_SMBR_LDS    1
#define PYCHAIN_HIP_SMBR_ROWS   2
#define PYCHAIN_HIP_SMBR_GLOBAL 3
int pychain_hip_smbr_form(int num_states, int num_pdfs, int num_classes, int requested);
size_t pychain_hip_smbr_general_lds_bytes(int num_states);
size_t pychain_hip_smbr_general_workspace_bytes(int B, int T, int num_states, int num_pdfs, int num_classes);
int pychain_hip_smbr_forward_backward_general(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* leaky_probs, const float* initial_probs, const float* final_probs,
    const int32_t* pdf_arcs, const int32_t* pdf_index, int num_states, int num_transitions,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    const int32_t* target_pdfs, const float* target_probs, int K, const float* frame_acc,
    float leaky_hmm_coefficient, float grad_scale, const float* grad_scale_dev,
    void* grad /* nnet_output_dtype */, double* acc_per_seq, float* closing, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream,
    const int32_t* pdf_classes, int num_classes, int targets_are_classes, int form);

/* ------------------------------------------------------------------------
 * Expected arc counts: the gradient of the denominator objective in the ARC WEIGHTS of its graph (ABI 30; DESIGN.md §3.29;
 * csrc/arc_counts.hip).  Let log Z_b(w) be the denominator objective of sequence b with every arc probability p_k replaced by
 * p_k exp(w_k), w = arc_log_weights in the order of forward_transitions (NULL: w = 0).  With x = exp(clamp(y, -30, 30)) and the
 * leaky HMM of the denominator, v' = v + c leaky sum(v) forwards and u' = u + c sum(leaky u) backwards,
 *
 *   post(b,t,k) = alpha'(t,src_k) p_k e^{w_k} x(t,pdf_k) beta'(t+1,dst_k) / (the same summed over the arcs)      sums to 1 over k
 *   c(b,k)      = d log Z_b / d w_k = sum_{t < L_b} post(b,t,k)                                                  sums to L_b over k
 *   gamma(b,t,n) = d log Z_b / d y(t,n) = the sum of post(b,t,k) over the arcs that carry pdf n
 *
 * - the expected number of times a path of the denominator takes arc k: the E-step statistics of the graph, and what training
 * the graph's weights (a learnable phone bigram, an LM or transition scale) needs.  At w = 0 log Z_b is the objective of
 * pychain_hip_den_forward_backward.  leaky_probs, initial_probs and final_probs are HELD FIXED: they are the caller's arrays, not
 * recomputed from the weighted graph and not differentiated; neither is the clamp.
 *
 * Arguments: the nine graph arrays in the reference layout and the arcs by pdf (pdf_arcs, pdf_index) as the sMBR entry points
 * take them; the backward arrays must hold the same arcs as the forward ones (an arc's backward copy finds its weight by its
 * endpoints, pdf and probability; arcs equal in all four pair up in order).  arc_log_weights: fp32 [num_transitions] or NULL; a
 * weight that is not finite is counted in bad_count[1] and taken as 0.  nnet_output [B,T,num_pdfs] in nnet_output_dtype, any
 * element-aligned start.  seq_weights: fp32 [B] or NULL (every u_b = 1).  Outputs:
 *   objf_per_seq    fp64 [B]: log Z_b; NaN for a sequence that went bad
 *   counts          fp64 [num_transitions]: sum_b u_b c(b,k)
 *   counts_per_seq  fp64 [B, num_transitions] or NULL: c(b,k), not weighted; zeros for a sequence that went bad
 *   grad            [B,T,num_pdfs] in nnet_output_dtype, or NULL (counts only): s u_b gamma(b,t,n), s = grad_scale
 *                   (* *grad_scale_dev where given); rows t >= L_b are exact zeros; a pdf no arc carries gets an exact zero and
 *                   its x is not read
 *   bad_count       int32 [2], zeroed by the call: [0] the sequences that went bad - a NaN in a live row, a frame total or a
 *                   frame divisor that is not positive and finite -, each counted once; [1] the weights that are not finite.
 * A bad sequence adds exact zeros to counts and leaves every other sequence's results bit-identical to a call where its
 * weight is 0.  No float atomics: fp32 vectors, every sum over time and over sequences in fp64 in a fixed order, so two calls
 * give the same bits; the 2-byte forms equal the fp32 form on the up-cast input, the gradient rounded once.
 * Launches: p exp(w) once; the recursions, 2B persistent workgroups with one state vector and the frame's row double-buffered in
 * LDS; the counts, time-parallel, a workgroup per run of 64 frames of a sequence with a partial row of num_transitions doubles;
 * log Z_b; the sums.  pychain_hip_den_arc_counts_lds_bytes(num_states, num_pdfs) = (2 H + 2 D + 64) * 4 + 256 must be within
 * 160 KiB: a larger graph is refused with PYCHAIN_HIP_EUNSUPPORTED and the sizes in the message (the general form: below).
 * Workspace: pychain_hip_den_arc_counts_workspace_bytes - the two trajectories, 8 (T+1) H B bytes, and B ceil(T / 64) partial rows.
 * pychain_hip_cpu_den_arc_counts: the host twin, the same equations with fp32 vectors, fp64 sums and host threads over the
 * sequences; fp32 rows and gradient. */
size_t pychain_hip_den_arc_counts_workspace_bytes(int B, int T, int num_states, int num_transitions);
size_t pychain_hip_den_arc_counts_lds_bytes(int num_states, int num_pdfs);
int pychain_hip_den_arc_counts(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* leaky_probs, const float* initial_probs, const float* final_probs,
    const int32_t* pdf_arcs, const int32_t* pdf_index, int num_states, int num_transitions,
    const float* arc_log_weights, const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    float leaky_hmm_coefficient, const float* seq_weights, float grad_scale, const float* grad_scale_dev,
    void* grad /* nnet_output_dtype */, double* objf_per_seq, double* counts, double* counts_per_seq, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream);
int pychain_hip_cpu_den_arc_counts(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* leaky_probs, const float* initial_probs, const float* final_probs,
    const int32_t* pdf_arcs, const int32_t* pdf_index, int num_states, int num_transitions,
    const float* arc_log_weights, const float* nnet_output, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    float leaky_hmm_coefficient, const float* seq_weights, float grad_scale, const float* grad_scale_dev,
    float* grad, double* objf_per_seq, double* counts, double* counts_per_seq, int32_t* bad_count, int num_threads);

/* ------------------------------------------------------------------------
 * Expected arc counts on graphs and trees beyond the LDS of a CU (ABI 31; csrc/arc_counts.hip).
 * pychain_hip_den_arc_counts keeps two state vectors and two rows of a frame in LDS and refuses num_states + num_pdfs > 20416:
 * 3000 states from about 17 400 pdfs, more than about 20 400 states at any num_pdfs.  The general kernels take any num_states,
 * num_pdfs and num_transitions the int32 layout holds, with the same equations, checks, outputs and workspace layout, between
 * the same launches (p exp(w) before; log Z_b and the sums behind); they are slower - what does not fit LDS is gathered from
 * global memory - and are asked for by name through an entry point of their own.  The forms are sMBR's, PYCHAIN_HIP_SMBR_*:
 *   LDS     the kernels of pychain_hip_den_arc_counts, launch for launch
 *   ROWS    the state vectors stay in LDS (pychain_hip_den_arc_counts_general_lds_bytes(num_states) within 160 KiB); the
 *           frame's row x of a recursion workgroup and the two rows x, x q0 of a count workgroup lie in scratch rows of the
 *           workspace; the counts run as at most 512 workgroups, persistent over the (sequence, run of 64 frames) items
 *   GLOBAL  the state vectors too are read back from the trajectories in the workspace: always runs
 *   AUTO    LDS where pychain_hip_den_arc_counts_lds_bytes is within 160 KiB, else ROWS where the state vectors fit, else GLOBAL
 * SAME BITS: thread-to-state and thread-to-pdf ownership, the arc order and the order of every sum are those of the LDS kernels,
 * so on a shape two forms take they give the same counts, counts_per_seq, objf_per_seq, grad and bad_count, bit for bit.  No
 * float atomics; a call gives the same bits every time.
 * pychain_hip_den_arc_counts_general_lds_bytes: the LDS of the ROWS form - one double-buffered state vector, the reduction
 *   scratch and the static LDS: (2 H + 64) * 4 + 256 bytes; 0 for num_states <= 0.
 * pychain_hip_den_arc_counts_form: host only; the form a call with `requested` would run, or PYCHAIN_HIP_EUNSUPPORTED (LDS or
 *   ROWS asked for on a shape it cannot hold: the sizes, the bytes and the budget are in the message) or PYCHAIN_HIP_EINVAL
 *   (sizes that are not positive, an unknown form).
 * pychain_hip_den_arc_counts_general_workspace_bytes: the layout of pychain_hip_den_arc_counts_workspace_bytes, then per
 *   recursion workgroup (2 B of them) and per count workgroup (min(B ceil(T / 64), 512)) a row of 2 num_pdfs floats rounded up
 *   to 64 floats, each region rounded up to 256 bytes; 0 for a size that is not positive.  A call whose form resolves to LDS
 *   needs pychain_hip_den_arc_counts_workspace_bytes only.
 * pychain_hip_den_arc_counts_general: the arguments of pychain_hip_den_arc_counts, then `form`; the same argument checks in
 *   the same order, made before the device is touched. */
size_t pychain_hip_den_arc_counts_general_lds_bytes(int num_states);
int pychain_hip_den_arc_counts_form(int num_states, int num_pdfs, int requested);
size_t pychain_hip_den_arc_counts_general_workspace_bytes(int B, int T, int num_states, int num_transitions, int num_pdfs);
int pychain_hip_den_arc_counts_general(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* leaky_probs, const float* initial_probs, const float* final_probs,
    const int32_t* pdf_arcs, const int32_t* pdf_index, int num_states, int num_transitions,
    const float* arc_log_weights, const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    float leaky_hmm_coefficient, const float* seq_weights, float grad_scale, const float* grad_scale_dev,
    void* grad /* nnet_output_dtype */, double* objf_per_seq, double* counts, double* counts_per_seq, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream, int form);

/* ------------------------------------------------------------------------
 * Expected arc counts of the NUMERATOR: the gradient of log P_b in per-sequence arc log-weights (ABI 32; DESIGN.md §3.31;
 * csrc/num_arcs.hip).  With every arc log-probability lp_k of sequence b's numerator graph replaced by fl32(lp_k + w(b,k)),
 * w = arc_log_weights [B, num_transitions] in the order of each sequence's forward_transitions,
 *
 *   c(b,k) = d log P_b / d w(b,k)
 *          = sum_{t < L_b} exp(alpha'(t,src_k) + lp_k + w(b,k) + x(t,pdf_k) + beta'(t+1,dst_k) - log P_b)      sums to L_b over k
 *
 * alpha', beta' and log P_b those of the weighted graph under the call's time windows (the recursions of
 * pychain_hip_num_forward_backward_tw), x = clamp(nnet_output, -30, 30).  initial_probs and final_probs are HELD FIXED and not
 * differentiated; neither is the clamp.  The expected number of times a path of the numerator takes arc k: which pronunciation
 * or optional-silence arc an utterance takes, how long it stays in each state, and - minus the counts of
 * pychain_hip_den_arc_counts - the LF-MMI gradient of a parameter that lives in both graphs.
 *
 * Arguments: those of pychain_hip_num_forward_backward_tw, with
 *   arc_log_weights  fp32 [B, num_transitions], any element-aligned start, or NULL.  Weights are per SEQUENCE also where the
 *                    graph is shared (graph_batch_stride 0): the call then keeps a copy per sequence of the graph in its workspace.
 *                    A weight that is not finite is counted in bad_count[1] and taken as 0.  Only the weights of a sequence's
 *                    used arcs - k < the largest forward_transition_indices[h][1] - are read.  The backward arrays must hold the
 *                    same arcs as the forward ones: an arc's backward copy finds its weight by (source, destination, pdf,
 *                    log-probability), and arcs equal in all four pair up in order, the r-th with the r-th.
 *   objf_per_seq     fp64 [B]: log P_b as the recursion found it (-inf without an admissible path, NaN where an arc emits one);
 *                    rounded to float it is the objf_per_seq of pychain_hip_num_forward_backward_tw
 *   grad             fp32 [B,T,num_pdfs] or NULL: the occupancies, as pychain_hip_num_forward_backward_tw writes them; NULL
 *                    skips the occupancy launch.  grad_mode: PYCHAIN_HIP_GRAD_LINEAR or _ACCUM; _LOG is PYCHAIN_HIP_EINVAL
 *   counts_per_seq   fp64 [B, num_transitions]: c(b,k); exact zeros for the arcs beyond a sequence's used arcs (batch padding)
 *                    and for a sequence whose log P_b is not finite - the other sequences' bits do not depend on it
 *   bad_count        int32 [2], zeroed by the call: [0] exactly what pychain_hip_num_forward_backward_tw counts for the same
 *                    call - with grad = NULL the occupancy checks do not run and only the recursion's verdicts (a log P_b that
 *                    is not finite, a length outside [1, T]) are counted; [1] the weights that are not finite
 * IDENTITIES: with arc_log_weights = NULL the graph's own buffers are read and no weight launch runs; with NULL and with all-zero
 * weights objf, grad and bad_count[0] are bit-identical to pychain_hip_num_forward_backward_tw on the same inputs.  Scattered by
 * pdf, c(b,.) is the sum over t of that call's LINEAR gradient rows.  No float atomics; two calls give the same bits.
 * Option num_compat = 1 (the reference's own arithmetic) takes no weights and leaves no log-shares: PYCHAIN_HIP_EUNSUPPORTED.
 * Launches: fl32(lp + w) in both arc orders (only with weights); the recursions and, with grad, the occupancy pass of
 * pychain_hip_num_forward_backward_tw on the substituted buffers; the counts, time-parallel - a workgroup per run of 64 frames of
 * a sequence, every arc with one owner thread, the posterior exp(fl32(alpha' + beta' - log P)(t,src_k) + r_k(t)) in fp32 from the
 * log-share r_k(t) the backward recursion stored, summed over the run in fp64 in ascending t into a partial row; the partial rows
 * of a sequence summed in ascending run.  Any num_states, num_transitions and num_pdfs the numerator takes.
 * pychain_hip_num_arc_counts_workspace_bytes: pychain_hip_num_workspace_bytes, then 8 B num_transitions bytes of weighted
 *   log-probabilities, a copy per sequence of the other graph arrays (24 B num_transitions + 24 B num_states bytes) and
 *   B ceil(T / 64) partial rows of num_transitions doubles; 0 for a size that is not positive; monotone in T.
 * pychain_hip_cpu_num_arc_counts: the host twin - pychain_hip_cpu_num_forward_backward_tw on fl32(lp + w), per-arc posteriors
 * summed in fp64, sequences on host threads; bad_count[0] counts sequences, as that twin does. */
size_t pychain_hip_num_arc_counts_workspace_bytes(int B, int T, int num_states, int num_transitions, int num_pdfs);
int pychain_hip_num_arc_counts(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions, int grad_mode, float grad_scale,
    const float* arc_log_weights, double* objf_per_seq, float* grad, double* counts_per_seq, int32_t* bad_count,
    void* workspace, size_t workspace_bytes, void* stream, const int32_t* time_windows);
int pychain_hip_cpu_num_arc_counts(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions, int grad_mode, float grad_scale,
    const float* arc_log_weights, double* objf_per_seq, float* grad, double* counts_per_seq, int32_t* bad_count,
    int num_threads, const int32_t* time_windows);

/* ------------------------------------------------------------------------
 * Fused ChainLoss (replaces the two ChainFunction calls + the autograd add of
 * pychain/loss.py:97-105 with one pass):
 *
 *   grad[b,t,n] = grad_scale * (gamma_den(b,t,n) - gamma_num(b,t,n))      written ONCE
 *   den_objf[b], num_objf[b] = per-sequence log-probabilities
 *
 * so that loss = -(sum num_objf - sum den_objf) [* grad_scale when the caller folds the
 * 1/sum(lengths) of `avg=True` into grad_scale] and d loss / d nnet_output = grad.
 * Numerically identical to calling the two entry points above and subtracting.
 *
 * Scheduling: the numerator recursion is independent of the denominator until the final
 * subtraction, so it runs CONCURRENTLY on a library-owned non-blocking side stream
 * (fork/join with events on `stream`; created once per device on first use, the only
 * hidden state of this library); the join precedes the sparse subtraction.
 * bad_count: dev int32[2] = {denominator, numerator}.
 * Arguments as in pychain_hip_den_forward_backward / pychain_hip_num_forward_backward.
 */
int pychain_hip_chain_loss_forward_backward(
    /* denominator */
    const void* plans_dev, int64_t plan_stride_bytes, int resident_slot_rows, int den_num_states,
    float leaky_hmm_coefficient,
    /* numerator */
    const int32_t* forward_transitions, const int32_t* forward_transition_indices,
    const float* forward_transition_probs, const int32_t* backward_transitions,
    const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    int num_num_states, int num_num_transitions,
    /* shared */
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs, float grad_scale,
    float* den_objf_per_seq, float* num_objf_per_seq, void* grad /* nnet_output_dtype */, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals,
    void* den_workspace, size_t den_workspace_bytes, void* num_workspace, size_t num_workspace_bytes,
    void* stream);

/* The same fused loss split at the autograd boundary (pychain/loss.py:27-87: forward returns
 * objf, backward returns input_grad * objf_grad):
 *
 *   _forward   runs the recursions (denominator alpha/beta + numerator alpha/beta, the latter on
 *              a side stream) and yields the per-sequence log-probabilities; the stored
 *              trajectories stay in the two workspaces, which the caller must keep untouched
 *              until _backward.  If `grad` is non-NULL the occupancy passes run as well,
 *              OVERLAPPED with the recursions (the frames whose alpha'/beta rows already exist
 *              are evaluated on the CUs the 2B persistent recursion workgroups leave idle), and
 *              grad = grad_scale * (gamma_den - gamma_num) is written; a caller that later
 *              learns an upstream gradient != 1 applies it with pychain_hip_rescale;
 *   _backward  runs the time-parallel occupancy passes and writes
 *              grad = grad_scale * (*grad_scale_dev) * (gamma_den - gamma_num) ONCE.
 *              grad_scale_dev (device float*, may be NULL = 1) is the upstream scalar gradient,
 *              read on the device: no host sync and no extra pass over [B,T,D] to apply it
 *              (the reference multiplies the stored gradient again, loss.py:85).
 * bad_count: dev int32[2] for _forward, dev int32[2] for _backward (may be the same words).
 * totals (dev float[PYCHAIN_HIP_TOTALS = 8] or NULL; _forward and _forward_backward): the scalars of ChainLoss.forward from the call's last
 *   kernel instead of from half a dozen scalar kernels of the host framework behind it (pychain/loss.py:100-104):
 *   totals[0] = (sum_b den_objf[b] - sum_b num_objf[b]) * loss_scale [/ *loss_norm_dev]  = -(num - den) [/ frames],
 *   totals[1] = sum_b len_b, totals[2] = bad_count[0] + bad_count[1] as a float (what a sharded trainer all-reduces
 *   with the loss), totals[3] = sum den - sum num unscaled, totals[4] = totals[0], totals[5..7] as above.  loss_norm_dev: device
 *   float or NULL; where it is given, a gradient written by the same call is divided by it too (grad = grad_scale /
 *   *loss_norm_dev * (gamma_den - gamma_num): the occupancy launches read its reciprocal on the device - ChainLoss(avg=True)
 *   with the lengths on the device costs no pass over [B,T,D] behind the call).
 * A batch larger than the chip (B >= 7/8 of the CU count, one shared denominator plan, `grad` given): the call runs over
 *   SLICES of about CUs / 2 sequences (B = 256: 2 x 128, 320: 2 x 160, 384: 3 x 128), one after the other on `stream` in the same workspaces (their last 4 KiB hold the
 *   slices' counters), and a last small launch forms bad_count and totals over the whole batch - same per-sequence results,
 *   same totals (fp64 over the per-sequence values, rounded once).  With every CU holding a recursion workgroup the
 *   numerator of ONE call only finds room as they end: B = 256 on 256 CUs 11.1 ms, as two slices 10.2.  Option
 *   "chain_slices": "0" never, "n" that many; pychain_hip_chain_loss_slices says what a call would do.
 */
int pychain_hip_chain_loss_slices(int64_t plan_stride_bytes, int resident_slot_rows, int B);
int pychain_hip_chain_loss_forward(
    const void* plans_dev, int64_t plan_stride_bytes, int resident_slot_rows, int den_num_states,
    float leaky_hmm_coefficient,
    const int32_t* forward_transitions, const int32_t* forward_transition_indices,
    const float* forward_transition_probs, const int32_t* backward_transitions,
    const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    int num_num_states, int num_num_transitions,
    const void* nnet_output, int nnet_output_dtype, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    float* den_objf_per_seq, float* num_objf_per_seq,
    void* grad /* may be NULL; nnet_output_dtype */, float grad_scale, int32_t* bad_count,
    float loss_scale, const float* loss_norm_dev, float* totals /* may be NULL */,
    void* den_workspace, size_t den_workspace_bytes, void* num_workspace, size_t num_workspace_bytes,
    void* stream);
/* ------------------------------------------------------------------------
 * Host twins (ABI 14): the same two computations on HOST pointers in the reference layout, for callers
 * whose tensors live on the CPU - the reference serves those from its own CPU loops (chain-computation.cc:113-176,247-311;
 * chain-log-domain-computation.cc:123-159,231-271) and code written against it unit-tests its criterion there.  The sequences
 * of the minibatch are dealt to `num_threads` host threads (0 = one per hardware thread); graph_batch_stride 0 = one graph
 * for every sequence, 1 = per-sequence graphs [B,...].  Denominator: fp32 state vectors and gradient, fp64 totals and
 * log-probability; numerator: fp64 log-probabilities, exact log-sum-exp (as the device path; the reference's fp32 LogAdd chain
 * is the device's option num_compat).  bad_count: host int32[1], the reference's `ok` (sequences whose log-probability is not
 * finite or whose frame-0 occupancies do not sum to one within 5 %).  These functions never touch a device, and the device
 * entry points never fall back to them.  pychain_hip_cpu_calls: how many host calls this process has made (the GPU tests
 * check that it stays where it was). */
long pychain_hip_cpu_calls(void);
int pychain_hip_cpu_den_forward_backward(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* leaky_probs, const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const float* nnet_output, int input_is_exp, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions,
    float leaky_hmm_coefficient, float grad_scale, float* objf_per_seq, float* grad, int32_t* bad_count, int num_threads);
int pychain_hip_cpu_num_forward_backward(
    const int32_t* forward_transitions, const int32_t* forward_transition_indices, const float* forward_transition_probs,
    const int32_t* backward_transitions, const int32_t* backward_transition_indices, const float* backward_transition_probs,
    const float* initial_probs, const float* final_probs, int graph_batch_stride,
    const float* nnet_output, const int64_t* seq_lengths,
    int B, int T, int num_pdfs, int num_states, int num_transitions, int grad_mode, float grad_scale,
    float* objf_per_seq, float* grad, int32_t* bad_count, int num_threads);

/* data[0..n) *= *scale_dev, skipped on the device when the scalar is exactly 1. */
int pychain_hip_rescale(void* data, int dtype /* PYCHAIN_HIP_F32 / _BF16 / _F16 */, size_t n, const float* scale_dev, void* stream);
/* 1 if the fused calls (_forward with a gradient or without, _forward_backward) take 2-byte network outputs for this shape:
 * both sides do (pychain_hip_den_half_native, pychain_hip_num_half_native) and the gradient is written ONCE, by the two-frame
 * occupancy kernel with the numerator folded in (an accumulation into a 2-byte gradient would round twice).
 * pychain_hip_chain_loss_backward is fp32 only. */
int pychain_hip_chain_loss_half_native(int64_t plan_stride_bytes, int resident_slot_rows, int den_num_states, int num_pdfs,
                                       int B, int T, int num_num_states, int num_num_transitions);
/* out[0] = (sum_b den_objf_per_seq[b] - sum_b num_objf_per_seq[b]) * scale, divided by *norm_dev if norm_dev != NULL:
 * the scalar ChainLoss.forward returns, -(num - den) [/ sum of lengths] (pychain/loss.py:100-104), in one launch
 * (fp64 accumulation, rounded once).  num_objf_per_seq may be NULL (denominator only).  All pointers on the device. */
int pychain_hip_loss_total(const float* den_objf_per_seq, const float* num_objf_per_seq, int B, float scale,
                           const float* norm_dev, float* out, void* stream);
/* NOT after a forward call that wrote its gradient in slices (a batch of >= 7/8 of the CU count with `grad` given:
 * pychain_hip_chain_loss_slices > 1): the workspaces then hold the LAST slice's trajectories only, and this call fails with
 * PYCHAIN_HIP_EUNSUPPORTED instead of writing a wrong gradient (the library remembers, by workspace address, which forward
 * call last wrote a workspace). */
int pychain_hip_chain_loss_backward(
    const void* plans_dev, int64_t plan_stride_bytes, int resident_slot_rows, int den_num_states,
    const int32_t* forward_transitions, const int32_t* forward_transition_indices,
    const float* forward_transition_probs,
    int graph_batch_stride, int num_num_states, int num_num_transitions,
    const void* nnet_output, int nnet_output_dtype /* PYCHAIN_HIP_F32 only */, const int64_t* seq_lengths, int B, int T, int num_pdfs,
    float grad_scale, const float* grad_scale_dev,
    void* grad, int32_t* bad_count,
    void* den_workspace, size_t den_workspace_bytes, void* num_workspace, size_t num_workspace_bytes,
    void* stream);

/* ------------------------------------------------------------------------
 * Batch containers (replaces the Python collation of pychain/graph.py:122-194).
 * The ten tensors of a ChainGraphBatch built from a list of graphs live in ONE buffer, fields in the order
 *   forward_transitions [B,K,3] i32, forward_transition_indices [B,H,2] i32, forward_transition_probs [B,K] f32,
 *   backward_transitions, backward_transition_indices, backward_transition_probs (same shapes),
 *   final_probs [B,H] f32, initial_probs [B,H] f32, leaky_probs [B,H] f32 (absent in the log domain), start_state [B] i64,
 * each field 64-byte aligned: _layout gives their byte offsets / bytes per utterance and returns the buffer size.
 *   _pack        host: rec[b] = {num_transitions, num_states, start_state, then the host addresses of the graph's nine
 *                tensors in field order (leaky = 0 in the log domain)}; pads as the reference does (zeros; -inf for
 *                initial / final probs in the log domain, graph.py:140-145).  Pack into pinned memory and the whole
 *                batch reaches the device with ONE copy.
 *   _reorder     host: out[b] = in[order[b]] for every field (index_select along the batch: graph.py:177-194; B_out may
 *                differ from B_in - sharding selects a subset)
 *   _reorder_dev the same gather between two DEVICE buffers, one launch on `stream`; order_dev: dev int64[B_out]. */
#define PYCHAIN_HIP_BATCH_FIELDS 10
#define PYCHAIN_HIP_BATCH_REC_WORDS 12
int64_t pychain_hip_batch_layout(int B, int K, int H, int log_domain, int64_t offsets[PYCHAIN_HIP_BATCH_FIELDS],
                                 int64_t row_bytes[PYCHAIN_HIP_BATCH_FIELDS]);
int     pychain_hip_batch_pack(int B, int K, int H, int log_domain, const uint64_t* rec, void* out, size_t out_bytes);
int     pychain_hip_batch_reorder(int B_in, int B_out, int K, int H, int log_domain, const void* in, void* out,
                                  const int64_t* order);
int     pychain_hip_batch_reorder_dev(int B_in, int B_out, int K, int H, int log_domain, const void* in_dev, void* out_dev,
                                      const int64_t* order_dev, void* stream);

/* ------------------------------------------------------------------------
 * Graph ingestion without OpenFST (host only, one-time per graph): what the reference's
 * `simplefst` module provides on top of OpenFST (openfst_binding/src/fstext.cc:174-184).
 * Handles are opaque host objects; *_read / *_from_arcs return NULL on error.
 *   pychain_hip_fst_read(file, 0)        StdVectorFst.read       (fstext.cc:178)
 *   pychain_hip_fst_read(file, offset)   StdVectorFst.read_ark   (ReadFstFromArk, fstext.cc:7-16)
 *   pychain_hip_fst_write                StdVectorFst.write      (fstext.cc:177)
 *   pychain_hip_fst_num_states / _start  num_states / start_state (fstext.cc:182-183)
 *   pychain_hip_fst_to_tensors           fst_to_tensor           (FstToTensor, fstext.cc:19-117)
 *   pychain_hip_fst_leaky_probs          set_leaky_probs         (SetLeakyProbs, fstext.cc:120-171)
 * fst_to_tensors outputs are caller-allocated: forward/backward transitions [K,3] int32, probs [K],
 * indices [H,2] int32, final [H]; K = pychain_hip_fst_num_arcs.
 */
void*   pychain_hip_fst_read(const char* filename, int64_t byte_offset);
void*   pychain_hip_fst_from_arcs(int32_t num_states, int32_t start, int64_t num_arcs,
                                  const int32_t* src, const int32_t* dst, const int32_t* ilabel,
                                  const float* weight, const float* final_weight);
void    pychain_hip_fst_free(void* fst);
int     pychain_hip_fst_write(const void* fst, const char* filename);
int32_t pychain_hip_fst_num_states(const void* fst);
int32_t pychain_hip_fst_start(const void* fst);
int64_t pychain_hip_fst_num_arcs(const void* fst);
int     pychain_hip_fst_to_tensors(const void* fst, int log_domain,
                                   int32_t* forward_transitions, float* forward_transition_probs,
                                   int32_t* forward_transition_indices,
                                   int32_t* backward_transitions, float* backward_transition_probs,
                                   int32_t* backward_transition_indices, float* final_probs);
int     pychain_hip_fst_leaky_probs(const void* fst, float* leaky_probs);

#ifdef __cplusplus
}
#endif
#endif  /* PYCHAIN_HIP_H_ */
