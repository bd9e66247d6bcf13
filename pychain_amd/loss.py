"""ChainFunction / ChainLoss: the LF-MMI autograd API of pychain on MI355X.

Mirror of the reference's pychain/loss.py (same names, signatures, defaults and
error behaviour).  What differs is underneath:

  * no extra passes over [B,T,D]: clamp(-30,30) and exp (loss.py:30,43) are fused
    into the HIP kernels, the log-domain gradient is produced in the linear
    domain directly (loss.py:77);
  * the denominator graph is compiled once to a device-resident plan that all B
    sequences share (no B-fold replication, no per-call H2D; graph.py:99-120,
    chain-computation.cc:77-89);
  * lengths may be given in any order and on any device (the reference needs
    them sorted descending on the CPU for pack_padded_sequence, loss.py:37-40);
  * fp16 / bf16 network outputs are accepted and read by the kernels AS THEY ARE (converted where they land, all
    arithmetic in fp32; the gradient is rounded to the input's dtype where it is written: no fp32 copy of [B,T,D]);
    the reference's C++ accessors take float32 only.

CPU tensors are served by the library's host twins (csrc/cpu.cpp), device tensors by the HIP kernels - never one for the
other: a device tensor that cannot reach the kernels raises.
"""
import torch
import torch.nn as nn

from . import _lib, _plan, native
from .graph import ChainGraphBatch

__all__ = ["ChainFunction", "ChainLossFunction", "ChainLossXentFunction", "NumeratorXentFunction", "numerator_xent",
           "output_regularizer", "weight_rows", "ChainLoss", "PosteriorTargets", "posterior_targets", "occupancies",
           "posterior_numerator", "PosteriorNumeratorFunction", "PosteriorChainLossFunction", "PosteriorChainLossXentFunction",
           "PosteriorXentFunction", "posterior_xent", "boost_rows", "BoostedDenominatorFunction"]


class ChainFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, input_lengths, graphs, leaky_coefficient=1e-5):
        B = input.size(0)
        if B != graphs.batch_size:
            raise ValueError(
                "input batch size ({}) does not equal to graph batch size ({})"
                .format(B, graphs.batch_size))
        x = input.detach()
        report = {}
        objf, input_grad, bad = ChainFunction._occupancies(x, input_lengths, graphs, leaky_coefficient, totals=True, report=report)
        return ChainFunction._forward_tail(ctx, input, x, input_lengths, graphs, leaky_coefficient, objf, input_grad, bad,
                                           report.get("totals"), report.get("per_seq"))

    @staticmethod
    def _occupancies(x, input_lengths, graphs, leaky_coefficient, totals=False, report=None):
        """(objf per sequence, occupancies = gradient for an upstream gradient of 1, bad_count).  `totals`: the
        denominator's last kernel also leaves [sum objf, frames, bad, sum objf, ...] (include/pychain_hip.h: totals) in
        `report["totals"]` - the caller attaches them to the tensor it returns - and the sum is returned in place of the
        per-sequence values (no reduction launch behind the call)."""
        D = x.size(2)
        # alignment time windows of a numerator batch (ChainGraphBatch.set_time_windows; objects without them: None)
        tw = getattr(graphs, "time_windows", None) if graphs.log_domain else None
        if not x.is_cuda:
            # CPU tensors: the library's host twins (pychain_amd/csrc/cpu.cpp) - what the reference does with them
            # (chain-computation.cc:40,136-175); device tensors never come here
            return native.cpu_forward_backward(graphs, x, input_lengths, leaky_coefficient, windows=tw)
        if not graphs.log_domain:   # usually the denominator
            if graphs.shared_graph is not None:
                plan = _plan.graph_plan(graphs.shared_graph, D, x.device)
            else:
                names = ("forward_transitions", "forward_transition_indices", "forward_transition_probs",
                         "backward_transitions", "backward_transition_indices", "backward_transition_probs",
                         "leaky_probs", "initial_probs", "final_probs")
                # keyed like graph_plan / device_tensors: an in-place edit or a replaced tensor re-compiles
                key = ("den_plans", str(x.device), D) + tuple(
                    (getattr(graphs, n).data_ptr(), getattr(graphs, n)._version) for n in names)
                hit = graphs._device_cache.get(key)
                if hit is None:
                    for k in [k for k in graphs._device_cache if k[:1] == ("den_plans",)]:
                        del graphs._device_cache[k]
                    hit = _plan.batch_plans({n: getattr(graphs, n) for n in names}, D, x.device)
                    graphs._device_cache[key] = hit
                plan = hit
            if totals:
                objf, input_grad, bad, tot = native.den_forward_backward(
                    plan, x, input_lengths, leaky_coefficient, input_is_exp=False, totals=True)
                if report is not None:
                    report["totals"], report["per_seq"] = tot, objf
                objf = native.totals_scalar(tot)   # (no launch; not a view of the statistics)
            else:
                objf, input_grad, bad = native.den_forward_backward(
                    plan, x, input_lengths, leaky_coefficient, input_is_exp=False)
        else:                       # usually the numerator
            gt = graphs.device_tensors(x.device)
            gstride = 0 if graphs.shared_graph is not None else 1
            objf, input_grad, bad = native.num_forward_backward(
                gt, gstride, graphs.num_states, x, input_lengths, grad_mode=_lib.GRAD_LINEAR,
                windows=None if tw is None else graphs.device_time_windows(x.device))
        return objf, input_grad, bad

    @staticmethod
    def _forward_tail(ctx, input, x, input_lengths, graphs, leaky_coefficient, objf, input_grad, bad, tot=None, per_seq=None):
        # The occupancies are the gradient for an upstream gradient of 1.  backward() scales the
        # buffer in place on the device (a no-op launch when the upstream gradient is exactly 1,
        # i.e. `objf.backward()`) and hands it to autograd, instead of the reference's extra
        # read+write pass over [B,T,D] (torch.mul, loss.py:85).  A SECOND backward over the same graph
        # (retain_graph=True; the reference allows it, loss.py:82-87) finds the buffer gone - autograd
        # owns it, it may be x.grad by now - and evaluates the occupancies again from the inputs kept
        # here by reference.  `retain_grad_buffer` = True keeps a private copy instead (reference cost).
        if ChainFunction.retain_grad_buffer:
            ctx.save_for_backward(input_grad)
        else:
            ctx.grad_buf = input_grad
            ctx.again = _recompute(x, lambda: ChainFunction._occupancies(x, input_lengths, graphs, leaky_coefficient),
                                   ChainFunction._grad_again)
        ctx.in_dtype = input.dtype   # fp16 / bf16 inputs are evaluated in fp32; the gradient goes back in their dtype
        out = objf.sum() if objf.dim() else objf               # (0-dim: the sum came with the call)
        # (internal: the [B] objectives the sum was taken over - what ChainLoss weights an unfused call's value with)
        out._objf_per_seq = objf if objf.dim() else per_seq
        return _attach(out, tot, bad)

    retain_grad_buffer = False
    # DEPRECATED mirrors of what the LAST call in this process reported (any criterion, any thread: two losses in one process
    # overwrite each other's).  Read `loss.totals` / `loss.totals_all` / `loss.bad_count` of the tensor a call RETURNED instead.
    last_totals = None           # device float[4] (include/pychain_hip.h: totals), None where the call produced none
    last_totals_all = None       # ... all eight: [5..7] say how a time-segmented call went (segments redone, count, worst mismatch)
    last_bad_count = None

    @staticmethod
    def _grad_again(result):
        """(of a re-evaluation's (objf, occupancies, bad_count): the occupancies; the bad count goes to the deprecated mirror)"""
        ChainFunction.last_bad_count = result[2]
        return result[1]

    @staticmethod
    def backward(ctx, objf_grad):
        # clamp is inside the Function and therefore not differentiated (loss.py:30,82-87)
        if ctx.saved_tensors:
            input_grad, = ctx.saved_tensors
            return torch.mul(input_grad, objf_grad).to(ctx.in_dtype), None, None, None
        return _grad_written_in_forward(ctx, objf_grad), None, None, None


def _attach(out, totals, bad):
    """What a call reports travels WITH the tensor it returns - `out.totals` (device float[4]: loss, frames, bad count, sum den - sum
    num; None where the call produced none), `out.totals_all` (all eight of include/pychain_hip.h), `out.bad_count` (device
    int32, the reference's `ok` as a count; never synced here) - so that two criteria, or two host threads, in one process do
    not read each other's.  The class attributes ChainFunction.last_* remain as deprecated mirrors."""
    out.totals = None if totals is None else totals[:4]
    out.totals_all = totals
    out.bad_count = bad
    ChainFunction.last_totals, ChainFunction.last_totals_all, ChainFunction.last_bad_count = out.totals, totals, bad
    return out


def _recompute(x, evaluate, pick):
    """The closure a second backward over a retained graph calls: evaluates again from the inputs kept by reference.
    autograd's version check only guards tensors saved with save_for_backward, so it is restated here: an in-place
    edit of the network output between the two backward calls would silently change the gradient (the reference
    saved the gradient itself, loss.py:79)."""
    version = x._version

    def again():
        if x._version != version:
            raise RuntimeError(
                "one of the variables needed for gradient computation has been modified by an inplace operation: "
                "the network output given to the LF-MMI loss is at version %d; expected version %d (second backward "
                "over a retained graph re-evaluates the loss from it)" % (x._version, version))
        return pick(evaluate())
    return again


def _take_grad_buffer(ctx, attr):
    """The gradient buffer written in forward, handed over ONCE (autograd then owns it: a leaf's
    .grad takes it without a copy); None when it is gone."""
    buf = getattr(ctx, attr, None)
    setattr(ctx, attr, None)
    return buf


def _grad_written_in_forward(ctx, upstream):
    """backward() of a Function whose forward wrote the gradient of its first input for an upstream gradient of 1 (ctx.grad_buf,
    ctx.again, ctx.in_dtype): the buffer, handed over once - a second backward over a retained graph evaluates again -,
    rescaled in place on the device (skipped there when the upstream gradient is exactly 1) or multiplied on the host
    (loss.py:85, as it is), in the input's dtype.  None where that input wants no gradient."""
    if not ctx.needs_input_grad[0]:
        return None
    grad = _take_grad_buffer(ctx, "grad_buf")
    if grad is None:
        grad = ctx.again()
    grad = native.rescale_(grad, upstream) if grad.is_cuda else torch.mul(grad, upstream)
    return grad.to(ctx.in_dtype)


def _with_output_reg(result, reg, speculative, host_scale, dev_norm, loss_scale):
    """`result` of native.chain_loss_forward with the output regularisers `reg` = (l2, oor) on top: native.output_reg on the
    current stream behind the fused call - ACCUM into the gradient the call wrote for an upstream gradient of 1 (speculative
    mode), else the objective only -, its scaled term added to the call's totals[0] and totals[4].  state.reg: the RegResult."""
    state, totals = result[3], result[4]
    state.reg = native.output_reg(state.x, state.lengths_dev, reg[0], reg[1], grad=state.grad if speculative else None,
                                  grad_mode=_lib.GRAD_ACCUM, grad_scale=host_scale, norm_dev=dev_norm, loss_scale=loss_scale,
                                  totals=totals)
    return result


def _attach_reg(out, res, reg, host_scale, dev_norm):
    """`out.l2_term`, `out.out_of_range_term`: the two amounts the regularisers added to the loss (detached, for logging)."""
    if res is None:
        return out
    l2t, oort = (0.5 * reg[0] * host_scale) * res.totals[1], (reg[1] * host_scale) * res.totals[2]
    if dev_norm is not None:
        l2t, oort = l2t / dev_norm.to(l2t.device), oort / dev_norm.to(oort.device)
    out.l2_term, out.out_of_range_term = l2t, oort
    return out


def _check_weights(utt_weights, deriv_weights, B, T, avg):
    """(u float32 [B] or None, f float32 [B,T] or None), each where it was given.  Weights on the host are inspected - negative or
    non-finite ones, and utterance weights that are all zero under `avg`, raise -; weights on the device are not (no sync)."""
    out = []
    for w, shape, what in ((utt_weights, (B,), "utt_weights"), (deriv_weights, (B, T), "deriv_weights")):
        if w is not None:
            w = torch.as_tensor(w).detach()
            if w.dtype != torch.float32:
                w = w.to(torch.float32)
            if tuple(w.shape) != shape:
                raise ValueError("%s must have shape %s, got %s" % (what, list(shape), list(w.shape)))
            if not w.is_cuda:
                if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                    raise ValueError("%s must be finite and not negative" % what)
                if avg and what == "utt_weights" and not bool((w != 0).any()):
                    raise ValueError("utt_weights are all zero: an averaged loss would divide by zero weighted frames")
        out.append(w)
    return tuple(out)


def _normaliser(avg, lengths, u=None):
    """(host scale, device normaliser) of a fused call: avg=True divides by N = the frame count (loss.py:103-104), or sum_b u_b
    L_b under utterance weights - a host scalar when everything it is made of lives on the host, else a device scalar; never a
    sync."""
    if not avg:
        return 1.0, None
    if u is None:
        if lengths.is_cuda:
            return 1.0, lengths.sum().to(torch.float32)
        return 1.0 / float(lengths.sum()), None
    if lengths.is_cuda or u.is_cuda:
        dev = u.device if u.is_cuda else lengths.device
        return 1.0, (u.to(dev).double() * lengths.to(dev)).sum().to(torch.float32)
    return 1.0 / float((u.double() * lengths).sum()), None


def _with_weights(result, wts, reg, c, speculative, dev_norm, loss_scale):
    """`result` of native.chain_loss_forward (with the regularisers' pass behind it, where there is one) under the weights `wts` =
    (u, f, ...), both on the call's device: native.weight_rows on the current stream - over the gradient the call wrote (speculative mode), over the xent
    branch's gradient, and, with utterance weights, the weighted sums into the call's totals.  state.weighted: the float[5]."""
    den_objf, num_objf, _, state, totals = result
    u, f = wts[:2]
    xe, rg = state.xent, state.reg
    if u is not None:
        l2, oor = reg if reg is not None else (0.0, 0.0)
        state.weighted = native.weight_rows(
            state.grad if speculative else None, state.lengths_dev, u, f, shape=state.shape[:3], den_objf=den_objf, num_objf=num_objf,
            xent_objf=None if xe is None else xe.objf, xent_coef=-c, reg_per_seq=None if rg is None else rg.per_seq, l2=l2, oor=oor,
            loss_scale=loss_scale, norm_dev=dev_norm, totals=totals)
    elif speculative:
        native.weight_rows(state.grad, state.lengths_dev, None, f)
    if xe is not None and xe.grad is not None:
        native.weight_rows(xe.grad, state.lengths_dev, u, f)
    return result


def _attach_weighted(out, state, totals, reg, host_scale, dev_norm):
    """`out.weighted_frames` = sum_b u_b L_b, and - under utterance weights - `out.xent_objf`, `out.l2_term`,
    `out.out_of_range_term` as the weighted amounts (detached, for logging)."""
    w = state.weighted
    if w is None:                                        # derivative weights only: they change no sum
        out.weighted_frames = totals[1]
        return out
    scaled = lambda t: t * host_scale if dev_norm is None else t * host_scale / dev_norm.to(t.device)
    out.weighted_frames = w[4]
    if state.xent is not None:
        out.xent_objf = scaled(w[1])
    if reg is not None:
        out.l2_term, out.out_of_range_term = scaled((0.5 * reg[0]) * w[2]), scaled(reg[1] * w[3])
    return out


class WeightRowsFunction(torch.autograd.Function):
    """Identity in forward; backward scales the rows of the incoming gradient by w(b,t) = u_b * f_bt over the live frames
    (include/pychain_hip.h: pychain_hip_weight_rows): device tensors on the HIP kernel, CPU tensors on the host twin."""

    @staticmethod
    def forward(ctx, input, lengths, u, f):
        ctx.lengths, ctx.u, ctx.f = lengths, u, f
        return input.view_as(input)

    @staticmethod
    def backward(ctx, g):
        if g.is_cuda:
            g = g.clone(memory_format=torch.contiguous_format)     # (autograd's buffer is not ours to write into)
            native.weight_rows(g, ctx.lengths, ctx.u, ctx.f)
            return g, None, None, None
        gf = g.to(torch.float32).clone(memory_format=torch.contiguous_format)
        native.cpu_weight_rows(gf, ctx.lengths, ctx.u, ctx.f)
        return gf.to(g.dtype), None, None, None


def weight_rows(x, weights, lengths=None):
    """x [B,T,D] unchanged in forward; in backward the rows of its gradient are scaled by `weights`: a [B] tensor (one weight per
    utterance), a [B,T] tensor (one per frame), or a pair (utterance weights, frame weights) - the row weight is then their fp32
    product, applied with ONE multiply.  Rows of weight 1 are not touched, rows of weight 0 are written as zeros without being
    read, rows t >= lengths[b] are left alone (`lengths` None: every frame is live).  The building block of ChainLoss's
    utt_weights / deriv_weights on the unfused route, and what a loss of one's own would call."""
    B, T = x.size(0), x.size(1)
    if isinstance(weights, (tuple, list)):
        u, f = weights
    else:
        weights = torch.as_tensor(weights)
        u, f = (weights, None) if weights.dim() == 1 else (None, weights)
    u, f = _check_weights(u, f, B, T, False)
    if u is None and f is None:
        raise ValueError("weight_rows: no weights given")
    if lengths is None:
        lengths = torch.full((B,), T, dtype=torch.int64)
    return WeightRowsFunction.apply(x, torch.as_tensor(lengths), u, f)


class _ValueOf(torch.autograd.Function):
    """value: `value` (detached); gradient: that of `local` (parallel.py's local - local.detach() + value, without the
    subtraction: a local loss that is not finite - an utterance of weight zero may make it so - must not make the value a NaN)."""

    @staticmethod
    def forward(ctx, local, value):
        return value.detach().to(local.dtype).clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _fused_forward(ctx, input, xent_output, input_lengths, den_graph, num_graphs, leaky_coefficient, avg, xent_regularize, reg, wts):
    """forward() of ChainLossFunction (`xent_output` None) and of ChainLossXentFunction: the fused call, behind it on the same
    stream the output regularisers' pass (`reg`) and the weights' pass (`wts`), each over the whole batch (after the last slice
    of a call in slices)."""
    x = input.detach()
    z = None if xent_output is None else xent_output.detach()
    B, D = x.size(0), x.size(2)
    if B != num_graphs.batch_size:
        raise ValueError(
            "input batch size ({}) does not equal to graph batch size ({})"
            .format(B, num_graphs.batch_size))
    lengths = torch.as_tensor(input_lengths)
    plan = _plan.graph_plan(den_graph, D, x.device)
    gt = num_graphs.device_tensors(x.device)
    gstride = 0 if num_graphs.shared_graph is not None else 1
    # (alignment time windows of the numerator, or None)
    tw = num_graphs.device_time_windows(x.device) if getattr(num_graphs, "time_windows", None) is not None else None
    # avg=True divides by the frame count (loss.py:103-104): a host scalar when the lengths
    # live on the host, else a device scalar - never a sync
    ctx.host_scale, ctx.dev_norm = _normaliser(avg, lengths, None if wts is None else wts[2])
    # When a gradient will be asked for, the occupancy passes run inside forward, overlapped
    # with the recursions, for an upstream gradient of 1 (what `loss.backward()` sends);
    # backward then only rescales if the upstream gradient turns out to differ.
    ctx.speculative = bool(ctx.needs_input_grad[0]) and ChainLossFunction.overlap
    # (2-byte network outputs go to the kernels as they are when the gradient is written here, or never)
    half_ok = ctx.speculative or not bool(ctx.needs_input_grad[0])
    spec, hscale, dnorm = ctx.speculative, ctx.host_scale, ctx.dev_norm      # (locals: the closures must not hold ctx)
    c = 0.0 if z is None else float(xent_regularize)
    xent = None if z is None else (z, bool(ctx.needs_input_grad[1]), c)

    def evaluate(loss_scale):
        r = native.chain_loss_forward(
            plan, gt, gstride, num_graphs.num_states, x, lengths, leaky_coefficient,
            with_grad=spec, grad_scale=hscale, loss_scale=loss_scale, norm_dev=dnorm, half_ok=half_ok, windows=tw, xent=xent)
        if reg is not None:
            # into the gradient the call wrote (speculative), else the objective only; behind the call's xent totals
            r = _with_output_reg(r, reg, spec, hscale, dnorm, loss_scale)
        if wts is not None:
            # the rows of the gradient the call wrote (speculative) and of the xent branch's, and the weighted sums into its totals
            r = _with_weights(r, wts, reg, c, spec, dnorm, loss_scale)
        return r
    den_objf, num_objf, bad, state, totals = evaluate(hscale)
    # a second backward over a retained graph (loss.py:82-87 allows it) runs the recursions again
    ctx.again = _recompute(x, lambda: evaluate(1.0), lambda r: (r[3], r[2]))   # (state, bad)
    ctx.reg, ctx.wts, ctx.state = reg, wts, state
    ctx.in_dtype = input.dtype
    ctx.z = z
    if z is not None:
        ctx.z_version, ctx.z_dtype = z._version, xent_output.dtype
    ctx.bad_count = bad                      # int32[2]: denominator, numerator; never synced here
    # -(num - den) [- c * xent] [/ frames], loss.py:100-104, comes with the call (the last workgroup of its last kernel adds the
    # per-sequence objectives up): no reduction / subtraction / scaling launches behind it
    objf = native.totals_scalar(totals)    # (no launch; not a view of the statistics: `loss /= n` works)
    out = _attach(objf, totals, bad)
    if z is not None:
        out.xent_objf = state.xent.totals[0]                # sum_b xent_objf[b] [/ frames]: detached, for logging
        out.xent_objf_per_seq = state.xent.objf
    out = _attach_reg(out, state.reg, reg, hscale, dnorm)
    return out if wts is None else _attach_weighted(out, state, totals, reg, hscale, dnorm)


def _fused_backward(ctx, objf_grad):
    """backward() of the two: (gradient of the chain output, gradient of the xent output), None where it is not wanted."""
    state = _take_grad_buffer(ctx, "state")
    if state is None:
        if ctx.z is not None and ctx.z._version != ctx.z_version:
            raise RuntimeError("one of the variables needed for gradient computation has been modified by an inplace operation: "
                               "the xent output given to the LF-MMI loss (second backward over a retained graph)")
        state, ctx.bad_count = ctx.again()
        ChainFunction.last_bad_count = ctx.bad_count
    grad = zgrad = None
    if ctx.needs_input_grad[0]:
        if ctx.speculative:
            # (a device-side normaliser - avg=True with the lengths on the device - was divided into the gradient by the call
            # that wrote it: include/pychain_hip.h, loss_norm_dev; an upstream gradient of exactly 1 then costs one tiny launch)
            grad = native.rescale_(state.grad, objf_grad)
        else:
            g = objf_grad if ctx.dev_norm is None else objf_grad / ctx.dev_norm.to(objf_grad.device)
            grad, bad = native.chain_loss_backward(state, ctx.host_scale, g)
            if ctx.reg is not None:
                # the regularisers' gradient into the one chain_loss_backward just wrote (scale host_scale * upstream)
                native.output_reg(state.x, state.lengths_dev, ctx.reg[0], ctx.reg[1], grad=grad, grad_mode=_lib.GRAD_ACCUM,
                                  grad_scale=ctx.host_scale, grad_scale_dev=g)
            if ctx.wts is not None:
                native.weight_rows(grad, state.lengths_dev, ctx.wts[0], ctx.wts[1])
            ctx.bad_count = ctx.bad_count + bad              # (the occupancy launches' own checks)
            ChainFunction.last_bad_count = ctx.bad_count
        grad = grad.to(ctx.in_dtype)
    if ctx.z is not None and ctx.needs_input_grad[1]:
        zgrad = native.rescale_(state.xent.grad, objf_grad).to(ctx.z_dtype)
    state.grad = state.xent = None         # the stored trajectories go with `state`
    state.den_ws = state.num_ws = None
    return grad, zgrad


class ChainLossFunction(torch.autograd.Function):
    """Denominator + numerator in one pass, split at the autograd
    boundary: forward runs the four recursions (numerator on a side stream) and returns the
    loss; backward runs the time-parallel occupancy passes and writes
    (gamma_den - gamma_num) * objf_grad [/ frames] ONCE, with the upstream gradient read on
    the device - instead of two dense gradients, two scalar multiplies and an autograd add
    (loss.py:85,100-104).  Same numbers as the two-call path."""

    @staticmethod
    def forward(ctx, input, input_lengths, den_graph, num_graphs, leaky_coefficient, avg, reg=None, wts=None):
        return _fused_forward(ctx, input, None, input_lengths, den_graph, num_graphs, leaky_coefficient, avg, 0.0, reg, wts)

    overlap = True     # class-level switch: False = occupancy passes run in backward (no speculation)

    @staticmethod
    def backward(ctx, objf_grad):
        return (_fused_backward(ctx, objf_grad)[0],) + (None,) * 7


class NumeratorXentFunction(torch.autograd.Function):
    """sum_b xent_objf[b] of include/pychain_hip.h (pychain_hip_xent): the numerator posteriors of (nnet_output, num_graphs) as
    cross-entropy targets of xent_output.  Differentiable in xent_output only - the posteriors are constant targets.  The
    gradient is written by the forward call for an upstream gradient of 1; backward rescales."""

    @staticmethod
    def forward(ctx, xent_output, nnet_output, lengths, num_graphs):
        x, z = nnet_output.detach(), xent_output.detach()
        if x.size(0) != num_graphs.batch_size:
            raise ValueError("input batch size ({}) does not equal to graph batch size ({})".format(x.size(0), num_graphs.batch_size))
        if not num_graphs.log_domain:
            raise ValueError("numerator_xent takes log-domain numerator graphs")
        z_grad = bool(ctx.needs_input_grad[0])
        evaluate = lambda: NumeratorXentFunction._evaluate(z, x, lengths, num_graphs, z_grad)
        res = evaluate()
        ctx.grad_buf = res.grad
        ctx.again = _recompute(z, evaluate, lambda r: r.grad)
        ctx.in_dtype = xent_output.dtype
        out = res.totals[1].clone()
        out.xent_objf_per_seq = res.objf
        return out

    @staticmethod
    def _evaluate(z, x, lengths, graphs, z_grad):
        tw = getattr(graphs, "time_windows", None)
        if not x.is_cuda:
            return native.cpu_num_xent(graphs, x, lengths, z, with_grad=z_grad, windows=tw)
        return native.num_xent(graphs.device_tensors(x.device), 0 if graphs.shared_graph is not None else 1, graphs.num_states,
                               x, lengths, z, with_grad=z_grad, windows=None if tw is None else graphs.device_time_windows(x.device))

    @staticmethod
    def backward(ctx, g):
        return _grad_written_in_forward(ctx, g), None, None, None


def numerator_xent(xent_output, nnet_output, lengths, num_graphs):
    """The cross-entropy objective of chain training's "xent regularisation" (Kaldi: --chain.xent-regularize): with gamma the
    numerator posteriors of (nnet_output, num_graphs) - under the batch's time windows, if set -
        sum_b sum_{t < L_b} sum_d gamma_b(t,d) log_softmax(xent_output)(b,t,d)
    as a 0-dim tensor, differentiable in xent_output only.  Device tensors run on the HIP kernels (one numerator
    forward-backward, compact posterior rows, one pass over xent_output), CPU tensors on the host twin.  `.xent_objf_per_seq`
    of the result: the [B] per-sequence objectives."""
    return NumeratorXentFunction.apply(xent_output, nnet_output, lengths, num_graphs)


class OutputRegFunction(torch.autograd.Function):
    """0.5 * l2 * sum_b R2_b + oor * sum_b RO_b of include/pychain_hip.h (pychain_hip_output_reg) as a 0-dim tensor, differentiable
    in the network output.  Device tensors: the LINEAR form of csrc/outreg.hip, the gradient written by the forward call for an
    upstream gradient of 1 (backward rescales); CPU tensors: the host twin."""

    @staticmethod
    def forward(ctx, input, lengths, l2, oor):
        x = input.detach()
        want = bool(ctx.needs_input_grad[0])
        run = native.output_reg if x.is_cuda else native.cpu_output_reg
        evaluate = lambda: run(x, lengths, l2, oor, grad_mode=_lib.GRAD_LINEAR, with_grad=want)
        res = evaluate()
        ctx.grad_buf = res.grad
        ctx.again = _recompute(x, evaluate, lambda r: r.grad)
        ctx.in_dtype = input.dtype
        out = res.totals[0].clone()
        out.l2_term, out.out_of_range_term = (0.5 * l2) * res.totals[1], oor * res.totals[2]
        out._reg_per_seq = res.per_seq                     # (internal: {R2_b, RO_b} [B,2], what ChainLoss weights the terms with)
        return out

    @staticmethod
    def backward(ctx, g):
        return _grad_written_in_forward(ctx, g), None, None, None


def output_regularizer(x, lengths, l2=0.0, out_of_range=0.0):
    """The two element-wise regularisers of the chain objective over the network output x [B,T,D] (Kaldi: --chain.l2-regularize,
    --chain.out-of-range-regularize), UN-averaged, as a 0-dim tensor differentiable in x:
        0.5 * l2 * sum x^2  +  out_of_range * sum max(|x| - 30, 0)^2        over the live frames t < lengths[b]
    (30 is the kernels' own clamp; frames beyond a length are never read and get a zero gradient).  `.l2_term` and
    `.out_of_range_term` of the result: the two amounts, detached."""
    l2, oor = float(l2), float(out_of_range)
    if l2 < 0.0 or oor < 0.0:
        raise ValueError("output_regularizer: l2 and out_of_range must not be negative (got %g, %g)" % (l2, oor))
    return OutputRegFunction.apply(x, lengths, l2, oor)


class PosteriorTargets(object):
    """Sparse per-frame posterior targets q(b,t,k) on the pdfs pdf(b,t,k) (include/pychain_hip.h: pychain_hip_post_targets): what
    ChainLoss.forward takes where the numerator graphs go when the supervision is a teacher's posteriors, or lattice posteriors
    of unlabelled audio.  `pdfs`: integer [B,T,K], -1 for padding; `probs`: float [B,T,K]; stored as int32 and float32.  Host
    tensors are validated (shapes, probs of the entries that are not padding finite and not negative; pdf < D where a call knows
    D); device tensors are not inspected (no sync)."""

    def __init__(self, pdfs, probs):
        pdfs, probs = torch.as_tensor(pdfs), torch.as_tensor(probs)
        if pdfs.dim() != 3 or tuple(pdfs.shape) != tuple(probs.shape) or pdfs.size(2) < 1:
            raise ValueError("PosteriorTargets: pdfs and probs must both be [B, T, K >= 1], got %s and %s"
                             % (list(pdfs.shape), list(probs.shape)))
        if pdfs.is_floating_point() or pdfs.dtype == torch.bool or not probs.is_floating_point():
            raise ValueError("PosteriorTargets: pdfs must be an integer tensor and probs a float tensor")
        self.pdfs = pdfs.detach().to(torch.int32).contiguous()
        self.probs = probs.detach().to(torch.float32).contiguous()
        if not self.probs.is_cuda:
            used = self.probs[self.pdfs.to(self.probs.device) >= 0] if not self.pdfs.is_cuda else self.probs
            if not bool(torch.isfinite(used).all()) or bool((used < 0).any()):
                raise ValueError("PosteriorTargets: probs must be finite and not negative")
        self._device_cache = {}

    @property
    def batch_size(self):
        return int(self.pdfs.size(0))

    @property
    def device(self):
        return self.pdfs.device

    @classmethod
    def _of(cls, pdfs, probs):
        t = cls.__new__(cls)                                   # (tensors this package made: not inspected again)
        t.pdfs, t.probs, t._device_cache = pdfs, probs, {}
        return t

    def to(self, device):
        """The targets on `device`: uploaded once and cached until a tensor is replaced or edited in place (as
        ChainGraphBatch.device_tensors caches the numerator graphs)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.pdfs.device == device and self.probs.device == device:
            return self
        key = (str(device), self.pdfs.data_ptr(), self.pdfs._version, self.probs.data_ptr(), self.probs._version)
        hit = self._device_cache.get(key)
        if hit is None:
            hit = PosteriorTargets._of(self.pdfs.to(device, non_blocking=True), self.probs.to(device, non_blocking=True))
            self._device_cache = {key: hit}
        return hit

    def index_select(self, idx):
        """The targets of the utterances `idx` (parallel.shard_batch)."""
        idx = torch.as_tensor(idx, dtype=torch.int64)
        return PosteriorTargets._of(self.pdfs.index_select(0, idx.to(self.pdfs.device)).contiguous(),
                                    self.probs.index_select(0, idx.to(self.probs.device)).contiguous())

    def to_classes(self, classes):
        """The same targets with every id mapped through `classes` (an integer tensor [D], pdf -> class): what
        expected_accuracy(..., classes=classes, targets_are_classes=True) takes.  Padding stays padding; a pdf out of range
        (>= D) stays out of range (>= max(classes) + 1)."""
        classes = torch.as_tensor(classes)
        if classes.dim() != 1 or classes.is_floating_point() or classes.dtype == torch.bool or classes.numel() < 1:
            raise ValueError("to_classes: classes must be an integer tensor [D]")
        cl = classes.detach().to(device=self.pdfs.device, dtype=torch.int64)
        D, C = int(cl.numel()), int(cl.max()) + 1
        ids = self.pdfs.to(torch.int64)
        mapped = cl[ids.clamp(0, D - 1)]
        out = torch.where(ids < 0, ids, torch.where(ids >= D, ids.clamp_min(C), mapped))
        return PosteriorTargets._of(out.to(torch.int32).contiguous(), self.probs)

    def check(self, B, T, D):
        """Against the network output [B,T,D] of a call: the shape, and - host tensors only - every pdf below D."""
        if tuple(self.pdfs.shape[:2]) != (B, T):
            raise ValueError("posterior targets are [%d, %d, K], the network output is [%d, %d, D]"
                             % (self.pdfs.size(0), self.pdfs.size(1), B, T))
        if not self.pdfs.is_cuda and bool((self.pdfs >= D).any()):
            raise ValueError("posterior targets name pdf %d, the network output has %d" % (int(self.pdfs.max()), D))
        return self

    @classmethod
    def from_dense(cls, post, lengths, k, floor=0.0, normalize=True):
        """The `k` largest posteriors of every live frame of `post` [B,T,D] that are >= `floor` (ties: the lower pdf), divided by
        their sum when `normalize` (include/pychain_hip.h: pychain_hip_topk_rows): device tensors - fp32, bf16 or fp16 as they
        are - on the HIP kernel, CPU tensors on the host twin."""
        post = post.detach()
        if post.dim() != 3:
            raise ValueError("from_dense: posteriors must be [B, T, D], got %s" % list(post.shape))
        k = int(k)
        if k < 1 or k > min(post.size(2), 64):
            raise ValueError("from_dense: k must be in [1, min(D, 64)], got %d (D = %d)" % (k, post.size(2)))
        if post.is_cuda:
            if post.dtype not in native._DTYPE_CODE:
                post = post.float()
            return cls._of(*native.topk_rows(post, lengths, k, floor, normalize))
        return cls._of(*native.cpu_topk_rows(post, lengths, k, floor, normalize))


    @classmethod
    def from_alignment(cls, ali):
        """Hard targets out of an alignment (align.viterbi_align): K = 1, pdfs = ali.pdfs[..., None] with -1 beyond a length and
        for the utterances that did not align (ali.ok False), probs = 1.  posterior_xent(z, lengths, these) is then frame
        cross-entropy against the alignment."""
        pdfs = ali.pdfs.detach()                                   # (-1 beyond a length already: align.viterbi_align)
        B, T = pdfs.shape
        dev = pdfs.device
        live = (pdfs >= 0) & ali.ok.to(dev).to(torch.bool)[:, None]
        pd = torch.where(live, pdfs.to(torch.int32), torch.full((), -1, dtype=torch.int32, device=dev))
        return cls._of(pd[..., None].contiguous(), torch.ones(B, T, 1, dtype=torch.float32, device=dev))


def occupancies(x, lengths, graphs, leaky_coefficient=1e-5):
    """The dense occupancies gamma(b,t,d) of (x, graphs) - what ChainFunction's backward hands out for an upstream gradient of 1 -
    as a [B,T,D] tensor, not differentiable: of a probability-domain graph (a ChainGraph or a ChainGraphBatch: the denominator
    posteriors) or of log-domain numerator graphs.  Rows beyond a length are zero."""
    from .graph import ChainGraph
    x = x.detach()
    if isinstance(graphs, ChainGraph):
        graphs = ChainGraphBatch(graphs, x.size(0))
    if x.size(0) != graphs.batch_size:
        raise ValueError("input batch size ({}) does not equal to graph batch size ({})".format(x.size(0), graphs.batch_size))
    with torch.no_grad():
        return ChainFunction._occupancies(x, lengths, graphs, leaky_coefficient)[1]


def posterior_targets(teacher_output, lengths, graphs, k, leaky_coefficient=1e-5, floor=0.0, normalize=True):
    """The teacher side of teacher-student LF-MMI: the occupancies of (teacher_output, graphs) - `occupancies` - cut down to
    their `k` largest per frame - PosteriorTargets.from_dense.  Not differentiable."""
    return PosteriorTargets.from_dense(occupancies(teacher_output, lengths, graphs, leaky_coefficient), lengths, k, floor, normalize)


class PosteriorNumeratorFunction(torch.autograd.Function):
    """sum_b num_b of include/pychain_hip.h (pychain_hip_post_targets), differentiable in the network output: the gradient -
    zeros plus the pass with s = 1 - is written by the forward call for an upstream gradient of 1; backward rescales."""

    @staticmethod
    def forward(ctx, input, lengths, targets):
        x = input.detach()
        targets.check(*x.shape)
        want = bool(ctx.needs_input_grad[0])
        evaluate = lambda: PosteriorNumeratorFunction._evaluate(x, lengths, targets, want)
        num, grad, bad = evaluate()
        ctx.grad_buf = grad
        ctx.again = _recompute(x, evaluate, lambda r: r[1])
        ctx.in_dtype = input.dtype
        out = num.sum(dtype=torch.float64).to(torch.float32)
        out.objf_per_seq = out._objf_per_seq = num
        out.bad_count = bad
        return out

    @staticmethod
    def _evaluate(x, lengths, targets, want):
        tg = targets.to(x.device)
        if x.is_cuda:
            xk = x if x.dtype in native._DTYPE_CODE else x.float()
            grad = torch.zeros_like(xk, memory_format=torch.contiguous_format) if want else None
            num, bad = native.post_targets(xk, lengths, tg.pdfs, tg.probs, grad=grad)
        else:
            grad = torch.zeros(x.shape, dtype=torch.float32) if want else None
            num, bad = native.cpu_post_targets(x, lengths, tg.pdfs, tg.probs, grad=grad)
        return num, grad, bad

    @staticmethod
    def backward(ctx, g):
        return _grad_written_in_forward(ctx, g), None, None


def posterior_numerator(x, lengths, targets):
    """The numerator of posterior-target supervision, sum_b sum_{t < L_b} sum_k q_k clamp(x(b,t,pdf_k), -30, 30), as a 0-dim tensor
    differentiable in x (the clamp is not differentiated, as in the rest of the library).  Device tensors run on the HIP kernel,
    CPU tensors on the host twin.  `.objf_per_seq` of the result: the [B] per-sequence values; `.bad_count`: the entries that
    name a pdf the network output does not have."""
    return PosteriorNumeratorFunction.apply(x, lengths, targets)


class PosteriorXentFunction(torch.autograd.Function):
    """sum_b xent_objf[b] of include/pychain_hip.h (pychain_hip_xent_targets): sparse targets as cross-entropy targets of
    xent_output.  Differentiable in xent_output only.  The gradient is written by the forward call for an upstream gradient of
    1; backward rescales, a second backward over a retained graph evaluates again."""

    @staticmethod
    def forward(ctx, xent_output, lengths, targets):
        z = xent_output.detach()
        targets.check(*z.shape)
        want = bool(ctx.needs_input_grad[0])
        evaluate = lambda: PosteriorXentFunction._evaluate(z, lengths, targets, want)
        res, bad = evaluate()
        ctx.grad_buf = res.grad
        ctx.again = _recompute(z, evaluate, lambda r: r[0].grad)
        ctx.in_dtype = xent_output.dtype
        out = res.totals[1].clone()
        out.xent_objf_per_seq = res.objf
        out.bad_count = bad
        return out

    @staticmethod
    def _evaluate(z, lengths, targets, want):
        tg = targets.to(z.device)
        if not z.is_cuda:
            return native.cpu_xent_targets(z, lengths, tg.pdfs, tg.probs, with_grad=want)
        zk = z if z.dtype in native._DTYPE_CODE else z.float()
        res, bad = native.xent_targets(zk, lengths, tg.pdfs, tg.probs, with_grad=want)
        return native.xent_add_totals(res), bad

    @staticmethod
    def backward(ctx, g):
        return _grad_written_in_forward(ctx, g), None, None


def posterior_xent(xent_output, lengths, targets):
    """The cross-entropy objective of a network output against sparse targets - PosteriorTargets: a teacher's or a lattice's
    posteriors (the xent term of teacher-student and semi-supervised chain training), or PosteriorTargets.from_alignment:
    frame cross-entropy against an alignment -
        sum_b sum_{t < L_b} sum_k q(b,t,k) log_softmax(xent_output)(b,t,pdf(b,t,k))
    as a 0-dim tensor, differentiable in xent_output only.  xent_output is read raw (no clamp), in its own dtype.  A live frame
    without an entry costs nothing: its row is not read.  Device tensors run on the HIP kernel (one pass over xent_output),
    CPU tensors on the host twin.  `.xent_objf_per_seq` of the result: the [B] per-sequence objectives; `.bad_count`: the
    entries that name a pdf xent_output does not have."""
    if not isinstance(targets, PosteriorTargets):
        raise ValueError("posterior_xent takes PosteriorTargets, got %s" % type(targets).__name__)
    return PosteriorXentFunction.apply(xent_output, lengths, targets)


def _posterior_forward(ctx, input, xent_output, input_lengths, den_graph, targets, xent_targets, leaky_coefficient, avg,
                       xent_regularize, reg, wts, boost=None):
    """forward() of PosteriorChainLossFunction (`xent_output` None) and of PosteriorChainLossXentFunction.  `boost` = (boost
    targets, b > 0) or None: the boosted denominator - native.boost_rows writes e = exp(clamp(x)) with the
    targeted elements scaled by exp(-b a), and the denominator call runs on e with input_is_exp; everything behind it reads the
    unboosted x as before."""
    x = native._kernel_tensor(input.detach())      # (once for every pass of the step: they all read the same rows)
    z = None if xent_output is None else xent_output.detach()
    B, T, D = x.shape
    targets.check(B, T, D)
    tg = targets.to(x.device)
    lengths = torch.as_tensor(input_lengths)
    plan = _plan.graph_plan(den_graph, D, x.device)
    hscale, dnorm = _normaliser(avg, lengths, None if wts is None else wts[2])
    L = _lib.lib()
    # (2-byte network outputs go to the kernels as they are wherever the denominator's kernel family takes them; else up-cast once)
    xk, _ = native._rows_as_given(x, lambda: L.pychain_hip_den_half_native(plan.stride, plan.slot_rows, int(plan.num_states), D, B, T))
    K = int(tg.pdfs.size(2))
    c = 0.0 if z is None else float(xent_regularize)
    if z is not None:
        if tuple(z.shape) != (B, T, D):
            raise ValueError("xent_output has shape %s, the chain output %s" % (tuple(z.shape), (B, T, D)))
        native._require_device(z, "xent_output")
        xent_targets.check(B, T, D)
        ztg = xent_targets.to(x.device)
        zk = z if z.dtype in native._DTYPE_CODE else z.float()
        z_grad = bool(ctx.needs_input_grad[1])

    btg = None if boost is None else boost[0].to(x.device)

    def evaluate(loss_scale):
        if btg is None:
            den_objf, grad, dbad, totals = native.den_forward_backward(plan, xk, lengths, leaky_coefficient, grad_scale=hscale, totals=True)
        else:
            e, bbad = native.boost_rows(xk, lengths, btg.pdfs, btg.probs, boost[1])
            den_objf, grad, dbad, totals = native.den_forward_backward(plan, e, lengths, leaky_coefficient, input_is_exp=True,
                                                                       grad_scale=hscale, totals=True)
        if dnorm is not None:
            native.rescale_(grad, torch.reciprocal(dnorm.to(grad.device)))
        if btg is not None and grad.dtype != xk.dtype:
            grad = grad.to(xk.dtype)          # (the boosted rows are fp32, so is their gradient: one cast for 2-byte x - §3.24)
        num_objf, tbad = native.post_targets(xk, lengths, tg.pdfs, tg.probs, grad=grad, grad_scale=-hscale, norm_dev=dnorm,
                                             den_objf=den_objf, loss_scale=loss_scale, totals=totals)
        st = native.ChainLossState()
        st.x, st.lengths_dev, st.grad, st.shape = xk, native._lengths_dev(lengths, x.device), grad, (B, T, D, K)
        st.xent = st.reg = st.weighted = None
        bads = [dbad, tbad]
        if z is not None:
            # the xent output's pass (its gradient for the scale -c [/ N]) and its term into the totals post_targets just wrote
            # (on the caller's stream: the same pass on a side stream beside the denominator call was measured and gained
            # nothing - DESIGN.md §3.23)
            xe, xbad = native.xent_targets(zk, lengths, ztg.pdfs, ztg.probs, with_grad=z_grad, grad_scale=-c * hscale, norm_dev=dnorm)
            st.xent = native.xent_add_totals(xe, xbad, loss_scale, dnorm, -c, totals)
            bads.append(xbad)
        if btg is not None:
            bads.append(bbad)
        r = (den_objf, num_objf, torch.cat(bads), st, totals)
        if reg is not None:
            r = _with_output_reg(r, reg, True, hscale, dnorm, loss_scale)
        if wts is not None:
            r = _with_weights(r, wts, reg, c, True, dnorm, loss_scale)
        return r
    _, _, bad, state, totals = evaluate(hscale)
    # a second backward over a retained graph runs the passes again
    ctx.again = _recompute(x, lambda: evaluate(1.0), lambda r: r[3])
    ctx.state = state
    ctx.in_dtype = input.dtype
    ctx.z = z
    if z is not None:
        ctx.z_version, ctx.z_dtype = z._version, xent_output.dtype
    out = _attach(native.totals_scalar(totals), totals, bad)     # bad_count int32[2]: denominator, targets [, xent targets]
    if z is not None:
        out.xent_objf = state.xent.totals[0]                     # sum_b xent_objf[b] [/ N]: detached, for logging
        out.xent_objf_per_seq = state.xent.objf
    out = _attach_reg(out, state.reg, reg, hscale, dnorm)
    return out if wts is None else _attach_weighted(out, state, totals, reg, hscale, dnorm)


def _posterior_backward(ctx, objf_grad):
    """backward() of the two: (gradient of the chain output, gradient of the xent output), None where it is not wanted."""
    want_z = ctx.z is not None and ctx.needs_input_grad[1]
    if not (ctx.needs_input_grad[0] or want_z):
        return None, None
    state = _take_grad_buffer(ctx, "state")
    if state is None:
        if ctx.z is not None and ctx.z._version != ctx.z_version:
            raise RuntimeError("one of the variables needed for gradient computation has been modified by an inplace operation: "
                               "the xent output given to the LF-MMI loss (second backward over a retained graph)")
        state = ctx.again()
    grad = zgrad = None
    if ctx.needs_input_grad[0]:
        grad = native.rescale_(state.grad, objf_grad).to(ctx.in_dtype)
    if want_z:
        zgrad = native.rescale_(state.xent.grad, objf_grad).to(ctx.z_dtype)
    state.grad = state.xent = None
    return grad, zgrad


class PosteriorChainLossFunction(torch.autograd.Function):
    """ChainLoss on device tensors with PosteriorTargets where the numerator graphs go: loss = (sum_b den_b - sum_b num_b) / N, its
    gradient (gamma_den - q) / N written ONCE by the forward call for an upstream gradient of 1 - the denominator call
    (native.den_forward_backward, scale 1 / N), behind it on the same stream native.post_targets into that gradient (scale
    -1 / N) and into that call's totals, then the regularisers' and the weights' passes exactly as the fused step applies them.
    ChainLossFunction.overlap has no effect here: the denominator call always writes its gradient.
    LENGTHS ON THE DEVICE: N is then a device scalar the denominator entry point does not take, so its gradient is written
    un-normalised and ONE native.rescale_ by 1 / N - one extra pass over [B,T,D] - puts it on the scale of the passes behind
    it, which all read N on the device."""

    @staticmethod
    def forward(ctx, input, input_lengths, den_graph, targets, leaky_coefficient, avg, reg=None, wts=None, boost=None):
        return _posterior_forward(ctx, input, None, input_lengths, den_graph, targets, None, leaky_coefficient, avg, 0.0, reg, wts,
                                  boost)

    @staticmethod
    def backward(ctx, objf_grad):
        return (_posterior_backward(ctx, objf_grad)[0],) + (None,) * 8


class PosteriorChainLossXentFunction(torch.autograd.Function):
    """PosteriorChainLossFunction with a second differentiable input, the xent branch's output z, trained by cross-entropy against
    `xent_targets` (usually the very targets of the numerator; include/pychain_hip.h: pychain_hip_xent_targets; DESIGN.md
    §3.23): loss = LF-MMI_KL - c * xent, both divided by N when `avg`.  Behind post_targets on the same stream:
    native.xent_targets writes z's gradient (scale -c [/ N], an upstream gradient of 1), native.xent_add_totals adds the term to
    the step's totals; backward rescales.  The gradient of the chain output is PosteriorChainLossFunction's, bit for bit."""

    @staticmethod
    def forward(ctx, input, xent_output, input_lengths, den_graph, targets, xent_targets, leaky_coefficient, avg, xent_regularize,
                reg=None, wts=None, boost=None):
        return _posterior_forward(ctx, input, xent_output, input_lengths, den_graph, targets, xent_targets, leaky_coefficient, avg,
                                  xent_regularize, reg, wts, boost)

    @staticmethod
    def backward(ctx, objf_grad):
        return _posterior_backward(ctx, objf_grad) + (None,) * 10


def boost_rows(x, lengths, targets, boost):
    """The rows the boosted denominator is evaluated on, as a fresh float32 [B,T,D] tensor, not differentiable:
    e = exp(clamp(x, -30, 30)) over the live frames, the elements `targets` (PosteriorTargets) address scaled by
    exp(-boost * q) - a pdf that occurs several times in a frame once, by the sum of its q.  Rows beyond a length are zero.
    Device tensors run on the HIP kernel (native.boost_rows), CPU tensors on the host twin."""
    if not isinstance(targets, PosteriorTargets):
        raise ValueError("boost_rows takes PosteriorTargets, got %s" % type(targets).__name__)
    x = x.detach()
    targets.check(*x.shape)
    tg = targets.to(x.device)
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    if x.is_cuda:
        xk = x if x.dtype in native._DTYPE_CODE else x.float()
        return native.boost_rows(xk, lengths, tg.pdfs, tg.probs, boost, out=out)[0]
    return native.cpu_boost_rows(x, lengths, tg.pdfs, tg.probs, boost, out=out)[0]


class BoostedDenominatorFunction(torch.autograd.Function):
    """sum_b den_b of the BOOSTED denominator, differentiable in the network output: ChainFunction on the
    denominator graph with every path's score lowered by boost * a(t, pdf_t), a = `targets`.  The boosted rows (native.boost_rows,
    or the host twin) go to the denominator as they are (input_is_exp); its occupancies are the gradient for an upstream
    gradient of 1.  What ChainLoss's unfused route and CPU tensors put in the denominator's place when boost > 0."""

    @staticmethod
    def forward(ctx, input, input_lengths, den_graph, targets, boost, leaky_coefficient=1e-5):
        x = input.detach()
        targets.check(*x.shape)
        evaluate = lambda: BoostedDenominatorFunction._occupancies(x, input_lengths, den_graph, targets, boost, leaky_coefficient)
        objf, input_grad, bad = evaluate()
        if ChainFunction.retain_grad_buffer:
            ctx.save_for_backward(input_grad)
        else:
            ctx.grad_buf = input_grad
            ctx.again = _recompute(x, evaluate, ChainFunction._grad_again)
        ctx.in_dtype = input.dtype
        out = objf.sum()
        out._objf_per_seq = objf
        return _attach(out, None, bad)

    @staticmethod
    def _occupancies(x, lengths, den_graph, targets, boost, leaky_coefficient):
        """(objf per sequence, occupancies of the boosted rows, bad_count: the denominator's + the pass's)"""
        tg = targets.to(x.device)
        if not x.is_cuda:
            e, bbad = native.cpu_boost_rows(x, lengths, tg.pdfs, tg.probs, boost)
            objf, grad, bad = native.cpu_forward_backward(ChainGraphBatch(den_graph, x.size(0)), e, lengths, leaky_coefficient,
                                                          input_is_exp=True)
            return objf, grad, bad + bbad
        plan = _plan.graph_plan(den_graph, x.size(2), x.device)
        xk = x if x.dtype in native._DTYPE_CODE else x.float()
        e, bbad = native.boost_rows(xk, lengths, tg.pdfs, tg.probs, boost)
        objf, grad, bad = native.den_forward_backward(plan, e, lengths, leaky_coefficient, input_is_exp=True)
        return objf, grad, bad + bbad

    @staticmethod
    def backward(ctx, objf_grad):
        if ctx.saved_tensors:
            input_grad, = ctx.saved_tensors
            return (torch.mul(input_grad, objf_grad).to(ctx.in_dtype),) + (None,) * 5
        return (_grad_written_in_forward(ctx, objf_grad),) + (None,) * 5


class ChainLossXentFunction(torch.autograd.Function):
    """ChainLossFunction with a second differentiable input, the xent branch's output z: the numerator posteriors of the step
    become its cross-entropy targets inside the same fused call (include/pychain_hip.h: pychain_hip_xent).
    loss = LF-MMI - c * xent, both divided by the frame count when `avg`.  The gradient of z is written by the forward call
    (scale -c [/ frames], an upstream gradient of 1); backward rescales.  The gradient of the chain output is
    ChainLossFunction's, bit for bit: nothing flows back to it through the posteriors."""

    @staticmethod
    def forward(ctx, input, xent_output, input_lengths, den_graph, num_graphs, leaky_coefficient, avg, xent_regularize, reg=None,
                wts=None):
        return _fused_forward(ctx, input, xent_output, input_lengths, den_graph, num_graphs, leaky_coefficient, avg,
                              xent_regularize, reg, wts)

    @staticmethod
    def backward(ctx, objf_grad):
        return _fused_backward(ctx, objf_grad) + (None,) * 8


class ChainLoss(nn.Module):
    """`xent_regularize` = c > 0 and `forward(..., xent_output=z)`: the loss is LF-MMI - c * xent, xent the cross-entropy objective
    of z against the numerator posteriors of the same step (numerator_xent); `loss.xent_objf` is that objective [/ frames],
    detached.  c = 0 or no xent_output: exactly the loss without it.
    `output_l2_regularize` = l2, `out_of_range_regularize` = r: the loss gains (0.5 * l2 * sum x^2 + r * sum max(|x| - 30, 0)^2)
    [/ frames] over the live frames of the network output (output_regularizer); `loss.l2_term` and `loss.out_of_range_term` are
    the two amounts, detached.  Both zero: exactly the loss without them, launch for launch.
    `forward(x, lengths, targets)` with a PosteriorTargets where the numerator graphs go: posterior-target supervision
    (teacher-student and semi-supervised LF-MMI), loss = (sum_b den_b - sum_b sum q clamp(x)) / N - _forward_targets.
    `boost` = b > 0: the boosted objective (LF-bMMI) - the denominator is evaluated with every path's score
    lowered by b times its per-frame agreement with a reference a(t, n), `forward(..., boost_targets=...)`:
        den = log sum_paths p(path) prod_t exp(clamp(x(t, pdf_t)) - b * a(t, pdf_t))
    (bMMI up to the constant b * T, which is dropped; the margin is applied behind the clamp).  `loss.boost` is b.  b = 0:
    exactly the loss without it, launch for launch."""

    def __init__(self, den_graph, leaky_coefficient=1e-5, avg=True, xent_regularize=0.0, output_l2_regularize=0.0,
                 out_of_range_regularize=0.0, boost=0.0):
        super(ChainLoss, self).__init__()
        self.boost = float(boost)
        if not (self.boost >= 0.0) or self.boost == float("inf"):
            raise ValueError("ChainLoss: boost must be finite and not negative (got %r)" % self.boost)
        self.den_graph = den_graph
        self.avg = avg
        self.leaky_coefficient = leaky_coefficient
        self.xent_regularize = float(xent_regularize)
        self.output_l2_regularize = float(output_l2_regularize)
        self.out_of_range_regularize = float(out_of_range_regularize)
        if self.output_l2_regularize < 0.0 or self.out_of_range_regularize < 0.0:
            raise ValueError("ChainLoss: output_l2_regularize and out_of_range_regularize must not be negative (got %g, %g)"
                             % (self.output_l2_regularize, self.out_of_range_regularize))
        self.fused = True   # one-pass kernel path; False = two ChainFunction calls as in the reference

    def _reg(self):
        """(l2, oor), or None where both are zero: the code path is then exactly the one without them"""
        if self.output_l2_regularize == 0.0 and self.out_of_range_regularize == 0.0:
            return None
        return (self.output_l2_regularize, self.out_of_range_regularize)

    def _on_kernels(self, x, num_graphs):
        return self.fused and x.is_cuda and not self.den_graph.log_domain and num_graphs.log_domain

    def _boost(self, x, num_graphs, boost_targets):
        """(boost targets, b) of a call with boost > 0, checked against the network output; None where boost == 0: the code path
        is then exactly the one without it."""
        if self.boost == 0.0:
            return None
        if boost_targets is None and isinstance(num_graphs, PosteriorTargets):
            boost_targets = num_graphs
        if boost_targets is None:
            raise ValueError("ChainLoss: boost > 0 with numerator graphs needs boost_targets, the reference the margin is measured "
                             "against - usually PosteriorTargets.from_alignment(viterbi_align(x, lengths, num_graphs))")
        if not isinstance(boost_targets, PosteriorTargets):
            raise ValueError("ChainLoss: boost_targets must be PosteriorTargets, got %s" % type(boost_targets).__name__)
        if self.den_graph.log_domain:
            raise ValueError("ChainLoss: boost > 0 needs a probability-domain denominator graph (a log-domain one has no "
                             "entry point that takes the boosted rows)")
        boost_targets.check(x.size(0), x.size(1), x.size(2))
        return (boost_targets, self.boost)

    def forward(self, x, x_lengths, num_graphs, xent_output=None, utt_weights=None, deriv_weights=None, xent_targets=None,
                boost_targets=None):
        """`boost_targets` (with boost > 0): the PosteriorTargets a(t, n) the margin is measured against.  With PosteriorTargets
        where the numerator graphs go they default to those; with numerator graphs they are required - usually
        `PosteriorTargets.from_alignment(viterbi_align(x, lengths, num_graphs))`.  Posterior supervision on device tensors keeps
        its one-call route: native.boost_rows in front of the denominator call, which then reads the boosted rows as they are
        (`loss.bad_count` gains a last word: the pass's own count).  Graph numerators take the unfused route - the boosted
        denominator (BoostedDenominatorFunction), then the numerator through ChainFunction -, with time windows, xent_output, the
        regularisers and the weights as that route has them; CPU tensors likewise, on the host twins.  Ignored when boost == 0.
        `xent_targets` (with PosteriorTargets where the numerator graphs go, and `xent_output`): the PosteriorTargets the xent
        output is trained against - usually the same object, `criterion(y, lengths, targets, xent_output=z, xent_targets=targets)`;
        the loss is LF-MMI_KL - c * xent (posterior_xent), `loss.bad_count` gains a third word, the xent entries that name a pdf
        z does not have.  Graph numerators bring their own posteriors: `xent_targets` with them raises.
        `utt_weights` u (float [B]; Kaldi: Supervision::weight) scale each utterance's objective, its derivatives and the
        normaliser: loss = sum_b u_b term_b / N with N = sum_b u_b L_b under avg=True (else 1), term_b the utterance's whole
        objective (LF-MMI, the xent term and the regularisers that are switched on).  An utterance with u_b == 0 contributes
        exactly 0 even where its own objective is -inf or a NaN (`utt_weights=viterbi_align(...).ok.float()` drops the
        utterances that do not align).  `deriv_weights` f (float [B,T]; Kaldi: --apply-deriv-weights) scale the derivative rows
        ONLY: they change neither the loss nor N, so WITH THEM THE GRADIENT IS DELIBERATELY NOT THE GRADIENT OF THE RETURNED
        SCALAR.  x.grad(b,t,:) - and the xent output's - is w(b,t) = u_b * f_bt times what the same call with the same N writes
        without weights: rows of weight 1 are not touched, rows of weight 0 are written as zeros without being read (a NaN in
        them is gone), the others get one multiply and one rounding (native.weight_rows, one pass behind the fused call).
        Where a bf16 / fp16 network output is up-cast for the call (rows that are no multiple of 8 pdfs, overlap = False, the
        unfused route) the call's gradient is fp32 until it is handed back: the weights multiply THAT, and the product is
        rounded to the output's dtype once - not the rounded 2-byte gradient a second time.
        Other dtypes are converted to float32; weights on the host that are negative or not finite raise, as do utterance
        weights that are all zero under avg=True; weights on the device are not inspected.  `loss.weighted_frames` is
        sum_b u_b L_b; `loss.totals[1]` holds it too, `loss.totals[3]` sum_b u_b (den_b - num_b), and `loss.xent_objf`,
        `loss.l2_term`, `loss.out_of_range_term` become the weighted amounts.  Both None: exactly the call without them."""
        reg = self._reg()
        z = xent_output if self.xent_regularize != 0.0 else None
        wts = None
        if utt_weights is not None or deriv_weights is not None:
            wts = _check_weights(utt_weights, deriv_weights, x.size(0), x.size(1), self.avg)
        boost = self._boost(x, num_graphs, boost_targets)
        if boost is not None:
            out = self._forward_boosted(x, x_lengths, num_graphs, xent_output, z, reg, wts, xent_targets, boost)
            out.boost = self.boost
            return out
        if isinstance(num_graphs, PosteriorTargets):
            return self._forward_targets(x, x_lengths, num_graphs, xent_output, reg, wts, xent_targets)
        if xent_targets is not None:
            raise ValueError("ChainLoss: xent_targets go with PosteriorTargets as the numerator (numerator graphs bring their own "
                             "posteriors: the xent term takes its targets from them)")
        if not self._on_kernels(x, num_graphs):
            return self._forward_separate(x, x_lengths, num_graphs, z, reg, wts)
        if wts is not None:
            # (uploaded once for every pass of the step; the utterance weights as they were given ride along: a host
            # normaliser is made of them)
            dev = lambda w: None if w is None else w.to(x.device, non_blocking=True)
            wts = (dev(wts[0]), dev(wts[1]), wts[0])
        if z is None:
            return ChainLossFunction.apply(x, x_lengths, self.den_graph, num_graphs, self.leaky_coefficient, self.avg, reg, wts)
        return ChainLossXentFunction.apply(x, z, x_lengths, self.den_graph, num_graphs, self.leaky_coefficient, self.avg,
                                           self.xent_regularize, reg, wts)

    def _forward_boosted(self, x, x_lengths, num_graphs, xent_output, z, reg, wts, xent_targets, boost):
        """boost > 0: posterior supervision keeps _forward_targets' routes, with the boosted rows in front of the denominator;
        graph numerators go through _forward_separate - existing entry points only - with the boosted denominator in the
        denominator's place."""
        if isinstance(num_graphs, PosteriorTargets):
            return self._forward_targets(x, x_lengths, num_graphs, xent_output, reg, wts, xent_targets, boost)
        if xent_targets is not None:
            raise ValueError("ChainLoss: xent_targets go with PosteriorTargets as the numerator (numerator graphs bring their own "
                             "posteriors: the xent term takes its targets from them)")
        return self._forward_separate(x, x_lengths, num_graphs, z, reg, wts, boost=boost)

    def _forward_targets(self, x, x_lengths, targets, xent_output, reg, wts, xent_targets=None, boost=None):
        """`targets`: PosteriorTargets where the numerator graphs go (teacher-student and semi-supervised LF-MMI; Kaldi's "KL"
        objective): loss = (sum_b den_b - sum_b num_b) / N with num_b = sum_{t < L_b} sum_k q_k clamp(x(b,t,pdf_k), -30, 30), plus
        the regularisers, under the weights, N as for graphs.  The gradient is (gamma_den - q) / N.  Device tensors with
        fused = True and a probability-domain denominator: PosteriorChainLossFunction; else the unfused route with
        posterior_numerator in the numerator's place.  The xent term needs targets of its own, `xent_targets` (posterior_xent):
        xent_output without them raises; with them, and xent_regularize != 0, the loss is LF-MMI_KL - c * xent."""
        if xent_targets is None:
            if xent_output is not None:
                raise ValueError("ChainLoss: xent_output together with PosteriorTargets is not supported (the xent term takes its "
                                 "targets from numerator graphs)")
        elif not isinstance(xent_targets, PosteriorTargets):
            raise ValueError("ChainLoss: xent_targets must be PosteriorTargets, got %s" % type(xent_targets).__name__)
        z = xent_output if self.xent_regularize != 0.0 and xent_targets is not None else None
        targets.check(x.size(0), x.size(1), x.size(2))
        if z is not None:
            if tuple(z.shape) != tuple(x.shape):
                raise ValueError("xent_output has shape %s, the chain output %s" % (tuple(z.shape), tuple(x.shape)))
            xent_targets.check(x.size(0), x.size(1), x.size(2))
        if not (self.fused and x.is_cuda and not self.den_graph.log_domain):
            return self._forward_separate(x, x_lengths, targets, z, reg, wts, xent_targets, boost)
        if wts is not None:
            dev = lambda w: None if w is None else w.to(x.device, non_blocking=True)
            wts = (dev(wts[0]), dev(wts[1]), wts[0])
        if z is None:
            return PosteriorChainLossFunction.apply(x, x_lengths, self.den_graph, targets, self.leaky_coefficient, self.avg, reg, wts,
                                                    boost)
        return PosteriorChainLossXentFunction.apply(x, z, x_lengths, self.den_graph, targets, xent_targets, self.leaky_coefficient,
                                                    self.avg, self.xent_regularize, reg, wts, boost)

    def _forward_separate(self, x, x_lengths, num_graphs, z, reg, wts, xent_targets=None, boost=None):
        """The unfused route and CPU tensors: two ChainFunction calls as in the reference, the cross-entropy term through
        numerator_xent (`z`; with PosteriorTargets as the numerator: posterior_xent against `xent_targets`), the regularisers through output_regularizer (`reg`), each where it is switched on.
        Under weights `wts` = (u, f) the gradient comes from the loss as it is, evaluated on weight_rows(x, w) - its backward
        scales the rows, once, after autograd has added the calls' gradients up.  Derivative weights alone change neither the
        loss nor N.  Under utterance weights the loss is evaluated un-averaged and divided by N = sum_b u_b L_b; its value is
        replaced by the weighted sum of the per-sequence objectives the calls leave (fp64, rounded once)."""
        u, f = wts if wts is not None else (None, None)
        lengths = torch.as_tensor(x_lengths)
        if wts is not None:
            x = WeightRowsFunction.apply(x, lengths, u, f)
            z = None if z is None else WeightRowsFunction.apply(z, lengths, u, f)
        avg = self.avg and u is None
        # (with the regularisers, the loss without them reads x through a view of its own: its calls' gradients are added up at
        # that view, as ChainLoss without the terms adds them, and x receives exactly two gradients - that sum and the term.  A
        # sum of two does not depend on which arrives first: x.grad is (the gradient without the terms) + the term, rounded once
        # more)
        xv = x if reg is None else x.view_as(x)
        if boost is None:
            den = ChainFunction.apply(xv, x_lengths, ChainGraphBatch(self.den_graph, x.size(0)), self.leaky_coefficient)
        else:
            den = BoostedDenominatorFunction.apply(xv, x_lengths, self.den_graph, boost[0], boost[1], self.leaky_coefficient)
        if isinstance(num_graphs, PosteriorTargets):
            num = posterior_numerator(xv, x_lengths, num_graphs)
        else:
            num = ChainFunction.apply(xv, x_lengths, num_graphs)
        objf = -(num - den)
        if avg:
            objf = objf / x_lengths.sum()
        if z is not None:
            if isinstance(num_graphs, PosteriorTargets):
                xent = posterior_xent(z, x_lengths, xent_targets)
                xent_bad = xent.bad_count
            else:
                xent = numerator_xent(z, xv, x_lengths, num_graphs)
            xent_per_seq = xent.xent_objf_per_seq
            if avg:
                xent = xent / x_lengths.sum()
            objf = objf - self.xent_regularize * xent
            xent_objf = xent.detach()
        if reg is not None:
            term = output_regularizer(x, x_lengths, reg[0], reg[1])
            l2t, oort, reg_per_seq = term.l2_term, term.out_of_range_term, term._reg_per_seq
            if avg:
                n = x_lengths.sum()
                term, l2t, oort = term / n, l2t / n, oort / n
            objf = objf + term
        if u is not None:
            den_per_seq, num_per_seq = den._objf_per_seq, num._objf_per_seq
            dev = den_per_seq.device
            ud, live = u.to(dev).double(), u.to(dev) != 0
            total = lambda t: torch.where(live, ud * t.to(dev).double(), torch.zeros_like(ud)).sum()     # (weight 0: skipped, not multiplied)
            frames = (ud * lengths.to(dev)).sum()
            n = frames if self.avg else torch.ones_like(frames)
            value = total(den_per_seq - num_per_seq)
            if z is not None:
                sx = total(xent_per_seq)
                value = value - self.xent_regularize * sx
                xent_objf = (sx / n).to(torch.float32)
            if reg is not None:
                s2, so = total(reg_per_seq[:, 0]), total(reg_per_seq[:, 1])
                value = value + 0.5 * reg[0] * s2 + reg[1] * so
                l2t, oort = (0.5 * reg[0] * s2 / n).to(torch.float32), (reg[1] * so / n).to(torch.float32)
            if self.avg:
                objf = objf / frames.to(torch.float32)
            objf = _ValueOf.apply(objf, (value / n).to(torch.float32))
            frames = frames.to(torch.float32)
        # (several native calls made this loss: none's totals are the step's - ShardedChainLoss finds none and all-reduces its own
        # three scalars; the two bad counts ride along as they are: no launch here)
        objf.totals = objf.totals_all = None
        ChainFunction.last_totals = ChainFunction.last_totals_all = None
        objf.bad_count = (den.bad_count, num.bad_count)
        if z is not None and isinstance(num_graphs, PosteriorTargets):
            objf.bad_count = objf.bad_count + (xent_bad,)
        if z is not None:
            objf.xent_objf = xent_objf
        if reg is not None:
            objf.l2_term, objf.out_of_range_term = l2t, oort
        if wts is not None:
            objf.weighted_frames = frames if u is not None else lengths.sum()
        return objf
