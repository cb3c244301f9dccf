"""Operator layer, BatchNorm-fused kernels: conv output -> BatchNorm2d('m') -> (P)LIF over T (eas_bn_lif_*), the CSPLayer branch
pair, channel joins, BatchNorm + SiLU of the real-valued blocks (eas_bn_silu_*).  Reference arithmetic: yolox/models/network_blocks.py:52-53
behind yolox/utils/utils_snn.py:16-58.  ``eas_snn_amd.ops`` re-exports everything here (``ops.<name>``).

Every form -- one layer, the pair on the two channel ranges of one convolution output, the grouped launch of ``ops_group`` -- is the SAME
layer step on a channel range [c0, c0 + Cc) of a convolution output: ``bn_state`` (what the module's BatchNorm does this call),
``_bn_stats`` (batch statistics), then ``_lif_fwd`` / ``_lif_bwd`` or ``_silu_fwd`` / ``_silu_bwd``.  The autograd Functions below only
say which tensors autograd sees and what an undifferentiated output costs."""
import collections
import ctypes as C
import functools

import torch

from . import _lib
from ._ctx import ctx as opctx
from ._lib import check, ptr, stream
from .ops_core import SG_PATAN, SURROGATE_IDS, _alpha_arg, _call, _dev, _eval_invstd, _f32c, _take_conv_stats, _timer_add, _timer_mark, bump_counter, dense, ghost, is_small_int, mark_small_int, new_planes, planes_of, to_planes

# ------------------------------------------------------------------------------------------------ BatchNorm state and statistics
# running_mean / running_var: the buffers the kernels read (eval) or update (training with momentum), else None.  replicas: number of
# identical copies the batch stands for (a stateless block run ONCE for T identical time steps, ``ops.replicated``): the statistics are
# unchanged by replication except for the sample count of the unbiased running variance.
BnState = collections.namedtuple('BnState', 'running_mean running_var batch_stats momentum eps replicas')


def bn_state(bn, replicas=None):
    """What BatchNorm module ``bn`` does in this call, as the kernels take it; bumps ``num_batches_tracked`` like F.batch_norm's caller
    (call it once per layer call).  replicas: default the current ``ops.replicated`` scope."""
    batch = bn.training or (bn.running_mean is None and bn.running_var is None)
    update = batch and bn.training and bn.track_running_stats
    if update:
        if bn.momentum is None:
            raise _lib.EasHipError('the fused BatchNorm kernels update running statistics with a momentum (momentum=None: cumulative average)')
        if bn.num_batches_tracked is not None:
            bump_counter(bn.num_batches_tracked)
    running = update or not batch
    return BnState(bn.running_mean if running else None, bn.running_var if running else None, bool(batch),
                   float(bn.momentum) if update else None, float(bn.eps), opctx.replicas if replicas is None else int(replicas))


def _bn_pending(partial, chunks, state, count, pitch):
    """statistics whose finalize (mean, invstd, running update) happens inside the consuming kernel"""
    update = state.momentum is not None
    return _lib.EasBnPending(partial, chunks, int(state.replicas), count, float(state.eps), float(state.momentum if update else 0.0),
                             ptr(state.running_mean) if update else None, ptr(state.running_var) if update else None, pitch)


# Convolution -> BatchNorm hand-over (eas_conv_fwd_stats, north_star's fused conv -> BN -> LIF step): inside ``conv_stats_scope`` a
# matrix-core convolution also leaves the per-channel sums of its output tile by tile, and the BN kernel that consumes exactly that
# tensor next adds them up instead of reading y once more (no eas_bn_stats_partial launch).  The slot holds the convolution output
# itself, so its address cannot be reused while the slot is valid; a BN call on anything else falls back to the statistics pass.
def _bn_stats(L, y, state, TN, c0, Cc, HW, y_ctot=0, keep_slot=False, handed=None):
    """(mean, invstd, pending, keep) of channels [c0, c0 + Cc) of the convolution output ``y`` (TN samples; y_ctot: its channel count
    when the range is not all of it, else 0).  Batch statistics: the producing convolution's tile sums -- ``handed`` over by
    ``conv_group``, or found in the slot of ``conv_stats_scope`` (kept there for a second range with ``keep_slot``) -- or the
    partial-sum launch; the consumer finalizes them (``pending``) and ``keep`` must live until it is enqueued.  Eval mode: the running
    statistics, pending None."""
    if not state.batch_stats:
        return state.running_mean, _eval_invstd(state.running_var, state.eps), None, None
    mean = torch.empty(Cc, dtype=torch.float32, device=y.device)
    invstd = torch.empty(Cc, dtype=torch.float32, device=y.device)
    count = float(TN) * HW
    if handed is not None:
        got = handed, handed.numel() // (2 * y_ctot)
    else:
        got = _take_conv_stats(y.data_ptr(), TN * HW, y_ctot if y_ctot else Cc, keep_slot)
    if got is not None:                      # no launch: the consumer adds the convolution's tile sums
        stats, nb = got
        return mean, invstd, _bn_pending(stats.data_ptr() + 16 * c0 * nb, nb, state, count, nb), stats
    ws = torch.empty(L.eas_bn_workspace_doubles(Cc), dtype=torch.float64, device=y.device)
    if opctx.call_log is not None:
        opctx.call_log.append(('eas_bn_stats_partial', (None, y_ctot, TN, Cc, HW, int(state.replicas))))
    t0 = _timer_mark()
    chunks = L.eas_bn_stats_partial(y.data_ptr() + 4 * c0 * HW, y_ctot, TN, Cc, HW, ptr(ws), stream())
    if chunks <= 0:
        check(chunks if chunks < 0 else -1, 'eas_bn_stats_partial')
    _timer_add('eas_bn_stats', t0, 4 * TN * Cc * HW)        # the statistics launch read y once
    return mean, invstd, _bn_pending(ptr(ws), chunks, state, count, 0), ws


def _channel_slice(g, Cc):
    """total channel count if the fp32 gradient ``g`` [.., Cc, H, W] (4-D or 5-D) is a 16-byte aligned channel slice of a contiguous
    wider tensor (what the backward of an in-place concatenation hands out): the kernels read it in place.  Cc if it is contiguous
    itself, else 0 (the caller makes a contiguous copy)."""
    if g.dtype != torch.float32 or g.dim() not in (4, 5):
        return 0
    if g.is_contiguous():
        return Cc
    st, (C_, H, W) = g.stride(), g.shape[-3:]
    pitch = st[-4]                           # elements per sample of the wider tensor
    if st[-1] != 1 or st[-2] != W or st[-3] != H * W or pitch % (H * W) or pitch // (H * W) <= C_ or g.data_ptr() % 16:
        return 0
    if g.dim() == 5 and st[0] != g.shape[1] * pitch:
        return 0
    return pitch // (H * W)


@functools.lru_cache(maxsize=None)
def _arg_names(fn):
    """names of the arguments of ``fn.forward`` behind ctx (a plain staticmethod: a decorator around it would hide them)"""
    code = fn.forward.__code__
    return code.co_varnames[1:code.co_argcount]


def _needs(ctx, fn, name):
    return ctx.needs_input_grad[_arg_names(fn).index(name)]


def _grads(fn, **named):
    """backward's result for ``fn``: the given gradients at the positions of the forward arguments of those names, None elsewhere"""
    names = _arg_names(fn)
    if not set(named) <= set(names):
        raise _lib.EasHipError(f'{fn.__name__}.forward has no argument {sorted(set(named) - set(names))} (its arguments: {names})')
    return tuple(named.get(n) for n in names)


# ------------------------------------------------------------------------------------------------ K4 (BN + LIF)
# One layer as its callers describe it.  state: BnState; v_in: membrane potential carried in, or None; sg_id / alpha: surrogate id and
# its slope (None in the single form's 'patan', whose learnable slope is a tensor argument); cat = (buffer [T,N,Ctot,H,W], first
# channel[, spike planes of the buffer]) or None; planes: the output as spike planes.  The single form's Function takes v_in and cat as
# tensor arguments (autograd sees them) and puts them into the struct before the layer step.
LifLayer = collections.namedtuple('LifLayer', 'state v_in k_const v_th v_reset flags sg_id alpha write_v cat planes')
_LifSaved = collections.namedtuple('_LifSaved', 'k_const v_th v_reset flags sg_id alpha batch_stats Cc c0')


def _lif_fwd(L, y, y_ctot, c0, dims, gamma, beta, w, lay, residual=None, residual_sp=None, want_mean=False, keep_slot=False):
    """BN + LIF over T on channels [c0, c0 + Cc) of the convolution output ``y`` (Cc = gamma's length; y_ctot as in ``_bn_stats``);
    dims = (T, N, H, W, bcast), bcast: y is ONE plane [N,..] shared by the T steps.  Output placement: a fresh tensor; channels
    cat[1].. of the buffer cat[0] (returned as a view: concatenation in place); lay.planes: bf16 spike planes next to a ghost (see
    ``ghost``), or the groups cat[1]/8.. of the planes cat[2] of a ghost buffer.  residual [T,N,Cc,H,W]: the output is spikes +
    residual (SEW shortcut), read from ``residual_sp`` when it is a ghost.  Returns (spikes, v_out, mean over T, planes), the tensors
    the backward needs and its ``_LifSaved``."""
    T, N, H, W, bcast = dims
    Cc, HW, dev = gamma.shape[0], H * W, y.device
    cat = lay.cat
    _dev(y, gamma, beta, lay.v_in, w)
    v_in = _f32c(lay.v_in)
    TN = N if bcast else T * N
    mean, invstd, pend, keep = _bn_stats(L, y, lay.state, TN, c0, Cc, HW, y_ctot, keep_slot)
    if residual is not None:
        assert not want_mean and residual.shape == (T, N, Cc, H, W)
        if residual_sp is not None:
            assert lay.planes and residual_sp.is_contiguous() and residual_sp.shape == (T, N, Cc // 8, HW, 8)
        else:
            assert not lay.planes
            residual = _f32c(residual)
    sp, ctot = None, 0
    if cat is not None:
        buf, cat_c0 = cat[0], cat[1]
        ctot = buf.shape[2]
        if lay.planes:
            sp_buf = cat[2]
            assert sp_buf.dtype == torch.bfloat16 and sp_buf.is_contiguous() and cat_c0 % 8 == 0 and sp_buf.shape == (T, N, ctot // 8, HW, 8)
            sp = sp_buf.narrow(2, cat_c0 // 8, Cc // 8)
        else:
            assert buf.is_contiguous() and buf.shape[:2] == (T, N) and buf.shape[3:] == (H, W)
        spikes = buf.narrow(2, cat_c0, Cc)
    elif lay.planes:
        sp = new_planes(T, N, Cc, H, W, dev)
        spikes = ghost((T, N, Cc, H, W), dev)
    else:
        spikes = torch.empty((T, N, Cc, H, W), dtype=torch.float32, device=dev)
    v_out = torch.empty((N, Cc, H, W), dtype=torch.float32, device=dev) if lay.write_v else None
    mo = torch.empty((N, Cc, H, W), dtype=torch.float32, device=dev) if want_mean else None
    _call('eas_bn_lif_fwd', (4 * TN + (2 if sp is not None else 4) * T * N) * Cc * HW, L.eas_bn_lif_fwd_ex, y.data_ptr() + 4 * c0 * HW, y_ctot,
          ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(v_in), ptr(v_out), ptr(w), lay.k_const, lay.v_th, lay.v_reset, lay.flags,
          None if sp is not None else ptr(spikes), ptr(mo), T, N, Cc, HW, int(bcast), C.byref(pend) if pend is not None else None,
          None if residual_sp is not None else ptr(residual), ctot, ptr(sp), ptr(residual_sp), 0, stream())
    del keep
    saved = _LifSaved(lay.k_const, lay.v_th, lay.v_reset, lay.flags, lay.sg_id, lay.alpha, lay.state.batch_stats, Cc, c0)
    return (spikes, v_out, mo, sp), (mean, invstd, gamma, beta, v_in, w), saved


def _lif_bwd(L, g_s, g_mean, y, y_ctot, gy, dims, tensors, sv, want_w, alpha_t=None, want_alpha=False):
    """backward of ``_lif_fwd``: writes channels [c0, c0 + Cc) of ``gy`` (shaped like y), returns (grad gamma, grad beta, grad w, grad
    alpha).  A gradient that is a channel slice of a concatenation's gradient is read in place."""
    T, N, HW, bcast = dims
    mean, invstd, gamma, beta, v_in, w = tensors
    Cc = sv.Cc
    ctot = 0
    if g_s is not None:
        ctot = _channel_slice(g_s, Cc)
        if ctot == 0:
            g_s = _f32c(g_s)
    g_mean = _f32c(g_mean)
    ggamma, gbeta = torch.empty_like(gamma), torch.empty_like(beta)
    gw = torch.empty_like(w) if want_w else None
    ws = torch.empty(L.eas_bn_workspace_doubles(Cc), dtype=torch.float64, device=y.device)
    nsteps = T * N * Cc * HW
    nbytes = 12 * nsteps if not bcast else 4 * (nsteps + 2 * N * Cc * HW)
    off = 4 * sv.c0 * HW
    head = (ptr(g_s), ctot, ptr(g_mean), y.data_ptr() + off, y_ctot, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(v_in), ptr(w),
            sv.k_const, sv.v_th, sv.v_reset, sv.flags)
    tail = (int(sv.batch_stats), gy.data_ptr() + off, ptr(ggamma), ptr(gbeta), ptr(gw), ptr(ws), T, N, Cc, HW, int(bcast), stream())
    ga = None
    if alpha_t is not None:
        ga = torch.empty_like(alpha_t) if want_alpha else None
        _call('eas_bn_lif_bwd', nbytes, L.eas_bn_lif_bwd_patan, *head, ptr(alpha_t), ptr(ga), *tail)
    else:
        _call('eas_bn_lif_bwd', nbytes, L.eas_bn_lif_bwd_ex, *head, sv.sg_id, sv.alpha, *tail)
    return ggamma, gbeta, gw, ga


class _BNLIFFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, gamma, beta, v_in, w, alpha, residual, cat_buf, cat_sp, residual_sp, lay, cat_c0, want_mean, t_bcast):
        """y: [T,N,C,H,W], or [N,C,H,W] standing for ``t_bcast`` identical time steps.  alpha: the learnable slope of 'patan', else None.
        cat_buf / cat_c0 / cat_sp: ``LifLayer.cat`` as tensor arguments.  Fourth result: the spike planes (lay.planes)."""
        ctx.set_materialize_grads(False)      # a result nobody differentiates arrives as None in backward, not as a zero tensor
        y = _f32c(y)
        if t_bcast:
            T, (N, _, H, W) = int(t_bcast), y.shape
        else:
            T, N, _, H, W = y.shape
        if alpha is not None:
            _dev(alpha)
        lay = lay._replace(v_in=v_in, cat=(cat_buf, cat_c0, cat_sp) if cat_buf is not None else None)
        outs, tensors, ctx.cfg = _lif_fwd(_lib.lib(), y, 0, 0, (T, N, H, W, bool(t_bcast)), gamma, beta, w, lay, residual, residual_sp, want_mean)
        ctx.save_for_backward(y, alpha, *tensors)
        ctx.dims = (T, N, H * W, bool(t_bcast))
        ctx.has_residual = residual is not None
        for v in (outs[1], outs[3]):
            if v is not None:
                ctx.mark_non_differentiable(v)
        return outs

    @staticmethod
    def backward(ctx, g_s, g_v, g_mean, _g_sp):
        y, alpha_t, *tensors = ctx.saved_tensors
        if g_s is None and g_mean is None:
            return _grads(_BNLIFFn, y=torch.zeros_like(y))
        gy = torch.empty_like(y)
        ggamma, gbeta, gw, ga = _lif_bwd(_lib.lib(), g_s, g_mean, y, 0, gy, ctx.dims, tensors, ctx.cfg,
                                         tensors[5] is not None and _needs(ctx, _BNLIFFn, 'w'), alpha_t, _needs(ctx, _BNLIFFn, 'alpha'))
        # d(spikes + residual)/d residual = identity: the same tensor, no copy
        return _grads(_BNLIFFn, y=gy, gamma=ggamma, beta=gbeta, w=gw, alpha=ga, residual=g_s if ctx.has_residual else None)


class _JoinFn(torch.autograd.Function):
    """The tensor whose channel slices were written in place by the producers of ``parts`` (concatenation without a copy):
    forward hands out ``buf`` itself, backward hands each producer its channel slice of the gradient as a view."""

    @staticmethod
    def forward(ctx, buf, *parts):
        ctx.sizes = [p.shape[-3] for p in parts]
        return buf.view_as(buf)

    @staticmethod
    def backward(ctx, g):
        outs, c = [], 0
        for n in ctx.sizes:
            outs.append(g.narrow(-3, c, n))
            c += n
        return (None,) + tuple(outs)


def join_channels(buf, *parts, sp_buf=None):
    """sp_buf: the spike planes of the whole concatenation (``buf`` is then a ghost; the producers of ``parts`` wrote their channel groups)"""
    out = _JoinFn.apply(buf, *parts)
    if all(is_small_int(p) for p in parts):
        mark_small_int(out)
        if sp_buf is not None:
            out._eas_sp = sp_buf
    return out


class _BNLIF2Fn(torch.autograd.Function):
    """Two BN+LIF layers on the two channel ranges of ONE convolution output y12 [T,N,Ca+Cb,H,W] (the 1x1 branches conv1 /
    conv2 of a CSPLayer computed by one convolution with concatenated weights): each reads its channel slice in place and
    the backward writes both slices of ONE gradient tensor, so the convolution's input gradient needs no addition of two
    branch gradients and its input is read once."""

    @staticmethod
    def forward(ctx, y12, gamma_a, beta_a, w_a, gamma_b, beta_b, w_b, lay_a, lay_b):
        ctx.set_materialize_grads(False)      # a result nobody differentiates arrives as None in backward, not as a zero tensor
        L = _lib.lib()
        y12 = _f32c(y12)
        T, N, Ct, H, W = y12.shape
        outs, tensors, ctx.cfgs = [], [], []
        c0 = 0
        for gamma, beta, w, lay in ((gamma_a, beta_a, w_a, lay_a), (gamma_b, beta_b, w_b, lay_b)):
            (spikes, v_out, _, sp), saved, cfg = _lif_fwd(L, y12, Ct, c0, (T, N, H, W, False), gamma, beta, w, lay, keep_slot=c0 == 0)
            outs += [spikes, v_out, sp]
            tensors += saved
            ctx.cfgs.append(cfg)
            c0 += cfg.Cc
        ctx.save_for_backward(y12, *tensors)
        ctx.dims = (T, N, H * W, False)
        for v in (outs[1], outs[2], outs[4], outs[5]):
            if v is not None:
                ctx.mark_non_differentiable(v)
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_sa, g_va, _g_ua, g_sb, g_vb, _g_ub):
        y12, *tensors = ctx.saved_tensors
        L = _lib.lib()
        gy12 = torch.empty_like(y12)
        res = []
        for i, g_s in enumerate((g_sa, g_sb)):
            saved, sv = tensors[6 * i:6 * i + 6], ctx.cfgs[i]
            if g_s is None:
                gy12.narrow(2, sv.c0, sv.Cc).zero_()
                res.append([torch.zeros_like(p) if p is not None else None for p in (saved[2], saved[3], saved[5])])
            else:
                res.append(_lif_bwd(L, g_s, None, y12, y12.shape[2], gy12, ctx.dims, saved, sv, saved[5] is not None)[:3])
        (gga, gba, gwa), (ggb, gbb, gwb) = res
        return _grads(_BNLIF2Fn, y12=gy12, gamma_a=gga, beta_a=gba, w_a=gwa, gamma_b=ggb, beta_b=gbb, w_b=gwb)


def bn_lif_pair(y12, a, b):
    """a / b: (gamma, beta, w, LifLayer) of the two layers; the 'patan' surrogate is not available here (callers keep such layers on
    ``bn_lif_multistep``).  Returns (spikes_a, v_a, spikes_b, v_b); with planes the spike tensors are ghosts that carry them
    (``planes_of``)."""
    sa, va, pa, sb, vb, pb = _BNLIF2Fn.apply(y12, a[0], a[1], a[2], b[0], b[1], b[2], a[3], b[3])
    if pa is not None:
        sa._eas_sp = pa
    if pb is not None:
        sb._eas_sp = pb
    return sa, va, sb, vb


def bn_lif_supported(y_seq, T):
    return y_seq.dim() == 5 and T <= 8 and (y_seq.shape[-1] * y_seq.shape[-2]) % 4 == 0


def bn_lif_multistep(y_seq, gamma, beta, running_mean, running_var, use_batch_stats, momentum, eps, v_in, w, k_const,
                     v_th, v_reset, flags, surrogate, alpha, want_mean=False, write_v=None, t_bcast=0, residual=None, cat=None,
                     planes=False):
    """Fused BatchNorm(step_mode='m') + multi-step LIF on the conv output y_seq [T,N,C,H,W]
    (or one plane [N,C,H,W] shared by ``t_bcast`` identical steps).  cat = (buffer, first channel[, planes of the buffer]);
    planes: write the output as spike planes -- the returned spike tensor is then a ghost that carries them (``planes_of``); a ghost
    residual is read from its planes."""
    if write_v is None:
        write_v = opctx.state_writeback
    # a broadcast frame stands for t_bcast identical steps
    state = BnState(running_mean, running_var, bool(use_batch_stats), None if momentum is None else float(momentum), float(eps),
                    int(t_bcast) if t_bcast else 1)
    sg_id = SURROGATE_IDS[surrogate] if isinstance(surrogate, str) else int(surrogate)
    C_ = y_seq.shape[-3]
    res_sp = planes_of(residual) if residual is not None else None
    cat_sp = cat is not None and len(cat) > 2 and cat[2] is not None
    if residual is not None and res_sp is None and (cat_sp or planes) and C_ % 8 == 0 and is_small_int(residual):
        res_sp = to_planes(residual)             # a shortcut that arrives as fp32 spikes next to an output kept as planes
    planes = bool(planes or cat_sp) and C_ % 8 == 0 and (residual is None or res_sp is not None) and (cat is None or cat_sp)
    if residual is not None and res_sp is not None and not planes:
        residual, res_sp = dense(residual), None              # fp32 output asked for: the shortcut as fp32 as well
    if cat_sp and not planes:
        raise _lib.EasHipError('a concatenation buffer kept as spike planes needs producers that write planes')
    alpha = _alpha_arg(sg_id, alpha)
    learn = sg_id == SG_PATAN
    lay = LifLayer(state, None, float(k_const), float(v_th), float(v_reset), int(flags), sg_id, None if learn else alpha, bool(write_v),
                   None, planes)
    spikes, v_out, mo, sp = _BNLIFFn.apply(y_seq, gamma, beta, v_in, w, alpha if learn else None, residual,
                                           cat[0] if cat is not None else None, cat[2] if planes and cat is not None else None,
                                           res_sp.contiguous() if res_sp is not None else None, lay,
                                           int(cat[1]) if cat is not None else 0, bool(want_mean), int(t_bcast))
    if sp is not None:
        spikes._eas_sp = sp
    return spikes, v_out, mo


# ------------------------------------------------------------------------------------------------ BN + SiLU
# One layer ready to launch, under the field names of the grouped launch's problem structs (``ops_group`` fills its arrays with them)
_SiluFwd = collections.namedtuple('_SiluFwd', [f for f, _ in _lib.EasBnSiluFwdProblem._fields_])
_SiluBwd = collections.namedtuple('_SiluBwd', [f for f, _ in _lib.EasBnSiluBwdProblem._fields_])


def _silu_fwd_problem(L, y, y_ctot, c0, gamma, beta, state, cat=None, keep_slot=False, handed=None):
    """One BatchNorm + SiLU layer on channels [c0, c0 + Cc) of the convolution output ``y`` [N,..,H,W]: (problem, out, (mean, invstd),
    keep); problem.pending is None in eval mode.  cat = (buffer [N,Ctot,H,W], first channel): the result is written as that channel
    range of the buffer and ``out`` is a view of it (concatenation in place); y_ctot / keep_slot / handed / keep as in ``_bn_stats``."""
    N, _, H, W = y.shape
    Cc, HW = gamma.shape[0], H * W
    _dev(y, gamma, beta)
    mean, invstd, pend, keep = _bn_stats(L, y, state, N, c0, Cc, HW, y_ctot, keep_slot, handed)
    if cat is not None:
        buf = cat[0]
        assert buf.is_contiguous() and buf.dtype == torch.float32 and buf.shape[0] == N and buf.shape[2:] == (H, W)
        out = buf.narrow(1, cat[1], Cc)
        ctot = buf.shape[1]
    else:
        out = torch.empty((N, Cc, H, W), dtype=torch.float32, device=y.device)
        ctot = 0
    return _SiluFwd(y.data_ptr() + 4 * c0 * HW, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(out), N, Cc, HW, ctot, y_ctot, pend), out, \
        (mean, invstd), keep


def _silu_fwd(L, y, y_ctot, c0, gamma, beta, state, cat, keep_slot=False):
    """``_silu_fwd_problem`` launched on its own; returns (out, (mean, invstd))"""
    p, out, stats, keep = _silu_fwd_problem(L, y, y_ctot, c0, gamma, beta, state, cat, keep_slot)
    _call('eas_bn_silu_fwd', 8 * p.N * p.C * p.HW, L.eas_bn_silu_fwd_ex, p.y, p.mean, p.invstd, p.gamma, p.beta, p.out, p.N, p.C, p.HW,
          C.byref(p.pending) if p.pending is not None else None, p.out_ctot, p.y_ctot, stream())
    del keep
    return out, stats


def _silu_bwd_problem(L, g, y, y_ctot, c0, mean, invstd, gamma, beta, batch_stats, gy):
    """backward of one BatchNorm + SiLU layer: (problem, grad gamma, grad beta, keep).  Writes channels [c0, c0 + Cc) of ``gy`` (shaped
    like y); the gradient of an in-place concatenation arrives as a channel slice of the concatenation's gradient and is read in place."""
    N, HW, Cc = y.shape[0], y.shape[2] * y.shape[3], gamma.shape[0]
    ctot = _channel_slice(g, Cc)
    if ctot == 0:
        g = _f32c(g)
    ggamma, gbeta = torch.empty_like(gamma), torch.empty_like(beta)
    ws = torch.empty(L.eas_bn_workspace_doubles(Cc), dtype=torch.float64, device=y.device)
    off = 4 * c0 * HW
    return _SiluBwd(ptr(g), y.data_ptr() + off, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), gy.data_ptr() + off, ptr(ggamma), ptr(gbeta),
                    ptr(ws), int(batch_stats), N, Cc, HW, ctot, y_ctot), ggamma, gbeta, (g, ws)


def _silu_bwd(L, g, y, y_ctot, c0, mean, invstd, gamma, beta, batch_stats, gy):
    """``_silu_bwd_problem`` launched on its own; returns (grad gamma, grad beta)"""
    p, ggamma, gbeta, keep = _silu_bwd_problem(L, g, y, y_ctot, c0, mean, invstd, gamma, beta, batch_stats, gy)
    _call('eas_bn_silu_bwd', 12 * p.N * p.C * p.HW, L.eas_bn_silu_bwd, p.grad_out, p.y, p.mean, p.invstd, p.gamma, p.beta, p.batch_stats,
          p.grad_y, p.grad_gamma, p.grad_beta, p.workspace, p.N, p.C, p.HW, p.grad_out_ctot, p.y_ctot, stream())
    del keep
    return ggamma, gbeta


class _BNSiLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, gamma, beta, state, cat_buf=None, cat_c0=0):
        """cat_buf [N,Ctot,H,W]: the result is written as channels cat_c0.. of it and returned as a view (concatenation in place)."""
        y = _f32c(y)
        out, (mean, invstd) = _silu_fwd(_lib.lib(), y, 0, 0, gamma, beta, state, (cat_buf, cat_c0) if cat_buf is not None else None)
        ctx.save_for_backward(y, mean, invstd, gamma, beta)
        ctx.batch_stats = state.batch_stats
        return out

    @staticmethod
    def backward(ctx, g):
        y, mean, invstd, gamma, beta = ctx.saved_tensors
        gy = torch.empty_like(y)
        ggamma, gbeta = _silu_bwd(_lib.lib(), g, y, 0, 0, mean, invstd, gamma, beta, ctx.batch_stats, gy)
        return _grads(_BNSiLUFn, y=gy, gamma=ggamma, beta=gbeta)


class _BNSiLU2Fn(torch.autograd.Function):
    """Two BN + SiLU layers on the two channel ranges of ONE convolution output y12 [N,Ca+Cb,H,W] (two real-valued convolutions that read
    the same input computed as one, ``conv2d_dual``): each reads its channel slice in place, the backward writes both slices of ONE
    gradient tensor -- the convolution's input gradient needs no addition of two branch gradients."""

    @staticmethod
    def forward(ctx, y12, gamma_a, beta_a, gamma_b, beta_b, state_a, state_b, cat_a, cat_b):
        ctx.set_materialize_grads(False)      # a result nobody differentiates arrives as None in backward, not as a zero tensor
        L = _lib.lib()
        y12 = _f32c(y12)
        Ct = y12.shape[1]
        outs, saved, ctx.cfgs = [], [], []
        c0 = 0
        for gamma, beta, state, cat in ((gamma_a, beta_a, state_a, cat_a), (gamma_b, beta_b, state_b, cat_b)):
            out, stats = _silu_fwd(L, y12, Ct, c0, gamma, beta, state, cat, keep_slot=c0 == 0)
            outs.append(out)
            saved += [*stats, gamma, beta]
            ctx.cfgs.append((state.batch_stats, c0))
            c0 += gamma.shape[0]
        assert c0 == Ct
        ctx.save_for_backward(y12, *saved)
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_a, g_b):
        y12, *saved = ctx.saved_tensors
        L = _lib.lib()
        gy12 = torch.empty_like(y12)
        res = []
        for i, g in enumerate((g_a, g_b)):
            mean, invstd, gamma, beta = saved[4 * i:4 * i + 4]
            batch_stats, c0 = ctx.cfgs[i]
            if g is None:
                gy12.narrow(1, c0, gamma.shape[0]).zero_()
                res.append((torch.zeros_like(gamma), torch.zeros_like(beta)))
            else:
                res.append(_silu_bwd(L, g, y12, y12.shape[1], c0, mean, invstd, gamma, beta, batch_stats, gy12))
        return _grads(_BNSiLU2Fn, y12=gy12, gamma_a=res[0][0], beta_a=res[0][1], gamma_b=res[1][0], beta_b=res[1][1])


def bn_silu_pair(y12, bn_a, bn_b, cat_a=None, cat_b=None):
    """(silu(bn_a(y12[:, :Ca])), silu(bn_b(y12[:, Ca:]))) for the output y12 of ``conv2d_dual``; cat_a / cat_b = (buffer, first channel)
    as in ``bn_silu``."""
    return _BNSiLU2Fn.apply(y12, bn_a.weight, bn_a.bias, bn_b.weight, bn_b.bias, bn_state(bn_a), bn_state(bn_b), cat_a, cat_b)


def bn_silu_supported(y):
    return y.is_cuda and y.dim() == 4 and y.dtype == torch.float32 and (y.shape[-1] * y.shape[-2]) % 4 == 0


def bn_silu(y, bn, cat=None):
    """silu(batch_norm(y)) for a plain ``nn.BatchNorm2d`` module ``bn`` (running statistics updated like F.batch_norm).
    cat = (buffer [N,Ctot,H,W], first channel): the result is written into that channel range of the buffer and returned as a view
    (the caller joins the buffer with ``join_channels``)."""
    state = bn_state(bn)
    if cat is not None:
        return _BNSiLUFn.apply(y, bn.weight, bn.bias, state, cat[0], cat[1])
    return _BNSiLUFn.apply(y, bn.weight, bn.bias, state)
