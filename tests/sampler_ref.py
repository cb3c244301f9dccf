"""Plain torch restatement of the adaptive sampler's state machine (K3, include/eas_hip.h: eas_arsnn_step_* / eas_arsnn_tail_* /
eas_arsnn_fused_step_fwd), written from the operation's definition -- the K3 header comment and the dense form of
oracle/embedding_ref.py -- for one micro-step GIVEN its convolution outputs.  dtype-generic; the tests use it in float64.  There is no
backward here: every gradient the tests compare with comes from torch.autograd on these forwards.
tests/test_cpu_sampler_ref.py pins it (in float32) to oracle.embedding_ref.AdaptiveRSNNEmbeddingRef, which the goldens pin to the
reference project.

The second half holds the case lists and the seeded input draws that tests/test_gpu_sampler_steps.py runs on the device and for which
tests/test_cpu_sampler_ref.py asserts the near-threshold caps: one definition, so the two cannot drift."""
import torch

READOUT = {'sum': 0, 'last': 1, 'avg': 2, 'running': 3}
MARGIN = 1e-4          # on u = vn - thresh: ten times the fp32 error bar of the comparison (1e-5)
TOL = 1e-5             # |got - ref| <= TOL * (1 + |ref|)


class _Rect(torch.autograd.Function):
    """Rectangle surrogate: forward [u > 0], backward g * alpha * [|u| < 0.5 / alpha]"""

    @staticmethod
    def forward(ctx, u, alpha):
        ctx.save_for_backward(u)
        ctx.alpha = alpha
        return (u > 0).to(u.dtype)

    @staticmethod
    def backward(ctx, g):
        u, = ctx.saved_tensors
        return g * ctx.alpha * (u.abs() < 0.5 / ctx.alpha).to(u.dtype), None


def rect(u, alpha=1.0):
    return _Rect.apply(u, alpha)


def near(u, alpha=1.0, margin=MARGIN):
    """True where an fp32 rounding of u may legitimately change a result: the spike itself (u ~ 0) and the edge of the surrogate's
    box (|u| ~ 0.5 / alpha)"""
    a = u.detach().abs()
    return (a < margin) | ((a - 0.5 / alpha).abs() < margin)


def _segment_write(agg, live, seg, val, Ts):
    """agg[seg] += val at the live elements; every other slot keeps its bits"""
    k = torch.arange(Ts, device=seg.device).view((Ts,) + (1,) * seg.dim())
    hit = live.unsqueeze(0) & (seg.unsqueeze(0) == k)
    return torch.where(hit, agg + val.unsqueeze(0), agg)


def step(g_in, c_in, g_rec, c_rec, v, vsum, seg, t_last, agg, t, Ts, readout, spike_attach, thresh, v_reset, spike_override=None, alpha=1.0):
    """One micro-step.  g_* / c_*: gate pre-activations / currents of the input and of the recurrent convolution; v, vsum: potential and
    running sum; seg (segments written so far, 0..Ts) and t_last (step of the last write, -1 = none) integer tensors; agg [Ts, ...].
    readout 0 sum, 1 last, 2 avg, 3 the plain gated recurrence (vsum never reset, no segment written).  v_reset None = soft reset.
    spike_override: a tensor whose non-NaN entries replace the FORWARD value of the spike (its gradient stays the surrogate's).
    -> (v_out, vsum_out, spike, gate, vn, seg_out, t_last_out, agg_out)"""
    readout = READOUT.get(readout, readout)
    gate = torch.sigmoid(g_in + g_rec)
    vn = gate * v + (c_in + c_rec)
    spike = rect(vn - thresh, alpha)
    if spike_override is not None:
        forced = torch.where(torch.isnan(spike_override), spike.detach(), spike_override.to(spike.dtype))
        spike = spike + (forced - spike.detach())
    v_out = vn - thresh * spike if v_reset is None else vn * (1 - spike) + v_reset * spike
    vs1 = vsum + vn
    if readout == 3:
        return v_out, vs1, spike, gate, vn, seg, t_last, agg
    fired = spike.detach() != 0
    live = fired & (seg < Ts)          # an element that has filled its Ts segments keeps firing, but its counter and t_last stay
    if readout == 0:
        val = vs1
    elif readout == 1:
        val = v_out
    else:
        val = vs1 / torch.where(live, t - t_last, torch.ones_like(t_last)).to(vs1.dtype)
    if spike_attach:
        val = val * spike
    agg_out = _segment_write(agg, live, seg, val, Ts)
    seg_out = seg + live.to(seg.dtype)
    t_last_out = torch.where(live, torch.full_like(t_last, t), t_last)
    vsum_out = torch.where(fired, torch.zeros_like(vs1), vs1)      # the sum restarts at EVERY fired element
    return v_out, vsum_out, spike, gate, vn, seg_out, t_last_out, agg_out


def tail(v, vsum, spike_last, seg, t_last, agg, Tm, Ts, readout, write_zero):
    """The write after the last step: elements that did not fire in it and still have a free segment add their readout (times zero with
    ``write_zero``) into agg[seg].  -> agg_out"""
    readout = READOUT.get(readout, readout)
    live = (spike_last.detach() == 0) & (seg < Ts)
    if readout == 0:
        val = vsum
    elif readout == 1:
        val = v
    else:
        val = vsum / torch.where(live, Tm - 1 - t_last, torch.ones_like(t_last)).to(vsum.dtype)
    if write_zero:
        val = val * 0
    return _segment_write(agg, live, seg, val, Ts)


def chain(X, Ts, readout, spike_attach, write_zero, use_abs, thresh, v_reset, running=None):
    """The whole state machine without convolutions: X [Tm, N, 2*C2, H, W], channels [0, C2) gate pre-activations, [C2, 2*C2) currents;
    ``step`` Tm times from the zero state, ``tail``, the optional ReLU.  running 'sum' | 'last': the plain gated recurrence instead
    (readout 3; the result is the running sum / the last potential).  -> (out, u [Tm, N, C2, H, W] = vn - thresh of every step)"""
    Tm, N, C, H, W = X.shape
    C2 = C // 2
    shape = (N, C2, H, W)
    z = torch.zeros(shape, dtype=X.dtype, device=X.device)
    v, vsum, spike = z, z, z
    seg = torch.zeros(shape, dtype=torch.int64, device=X.device)
    t_last = torch.full_like(seg, -1)
    agg = torch.zeros((Ts,) + shape, dtype=X.dtype, device=X.device)
    us = []
    for t in range(Tm):
        v, vsum, spike, _, vn, seg, t_last, agg = step(X[t, :, :C2], X[t, :, C2:], z, z, v, vsum, seg, t_last, agg, t, Ts,
                                                       3 if running else readout, spike_attach, thresh, v_reset)
        us.append((vn - thresh).detach())
    if running:
        out = vsum if running == 'sum' else v
    else:
        out = tail(v, vsum, spike, seg, t_last, agg, Tm, Ts, readout, write_zero)
    if use_abs:
        out = torch.relu(out)
    return out, torch.stack(us)


# ---------------------------------------------------------------------------------------------------------------------------------
# Cases and seeded draws shared by the device tests and the CPU cap test.  Everything is drawn on the CPU in float32 / int8 (what the
# kernels receive); the fp64 reference sees exactly these values.

THRESH = float(torch.tensor(0.9, dtype=torch.float32))       # the value the kernels receive for thresh = 0.9
RESETS = (None, 0.25, 0.0)                                   # soft, hard to 0.25, hard to 0
OPTIONS = [(r, sat, vr) for r in (0, 1, 2, 3) for sat in (0, 1) for vr in RESETS]      # readout x spike_attach x reset
STEP_SHAPES = [(3, 3, 108), (1, 1, 4), (2, 2, 16 * 64)]      # (N, C2, HW)
STEP_T_TS = [(0, 1), (0, 3), (3, 1), (3, 3)]                 # (t, Ts)
WRAP_SHAPE = (2, 2, 1024 * 2056)                             # N * C2 * HW just above 8192 blocks * 256 threads * 4 elements
CAP_STEP, CAP_BWD, CAP_CHAIN = 1e-3, 0.0, 1e-2               # allowed share of near-threshold elements: groups A / E, B, D
BWD_SEED = 21                                                # float inputs of the step backward (groups B, C1)

# seed of the float inputs per (shape, thresh): u depends on nothing else.  If a seed exceeds its cap, change the seed, not the cap.
STEP_SEEDS = {((3, 3, 108), THRESH): 41, ((1, 1, 4), THRESH): 12, ((2, 2, 1024), THRESH): 13, ((3, 3, 108), 1.0): 34,
              ((1, 1, 64), THRESH): 15, (WRAP_SHAPE, THRESH): 16}


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def draw_state(g, shape, t, Ts, seg_values=None, tl_values=None):
    """A consistent prior state: seg from 0..Ts INCLUDING Ts (a frozen element), t_last = -1 exactly where seg == 0 and from 0..t-1
    elsewhere.  Before step 0 nothing can have been written: seg = 0 everywhere.  seg_values / tl_values: draw from these lists."""
    if t == 0:
        return torch.zeros(shape, dtype=torch.int8), torch.full(shape, -1, dtype=torch.int8)
    if seg_values is None:
        seg = torch.randint(0, Ts + 1, shape, generator=g)
    else:
        seg = torch.tensor(seg_values)[torch.randint(0, len(seg_values), shape, generator=g)]
    if tl_values is None:
        tl = torch.randint(0, t, shape, generator=g)
    else:
        tl = torch.tensor(tl_values)[torch.randint(0, len(tl_values), shape, generator=g)]
    tl = torch.where(seg == 0, torch.full_like(tl, -1), tl)
    return seg.to(torch.int8), tl.to(torch.int8)


def draw_step(shape, thresh):
    """float inputs of one step: conv_in / conv_rec [N, 2*C2, HW] (gate pre-activations | currents), v, vsum [N, C2, HW]"""
    N, C2, HW = shape
    g = _gen(STEP_SEEDS[(tuple(shape), thresh)])
    conv_in = torch.randn(N, 2 * C2, HW, generator=g)
    conv_in[:, C2:] = 0.8 * conv_in[:, C2:] + 0.5
    conv_rec = 0.5 * torch.randn(N, 2 * C2, HW, generator=g)
    v = 0.7 * torch.randn(N, C2, HW, generator=g) + 0.3
    vsum = torch.randn(N, C2, HW, generator=g)
    return conv_in, conv_rec, v, vsum


def step_u(conv_in, conv_rec, v, thresh):
    """u = vn - thresh of a step in float64 (v None: the first step)"""
    C2 = conv_in.shape[1] // 2
    ci, cr = conv_in.double(), conv_rec.double()
    gate = torch.sigmoid(ci[:, :C2] + cr[:, :C2])
    vn = ci[:, C2:] + cr[:, C2:]
    if v is not None:
        vn = gate * v.double() + vn
    return vn - thresh


def draw_bwd(shape, thresh, seed=BWD_SEED):
    """what the step backward receives: gate, vn as the forward saved them (float32), the prior v / vsum and the four incoming gradients.
    vn is drawn so that NO element is near a threshold (the few that are get redrawn): a condition on the inputs alone."""
    N, C2, HW = shape
    g = _gen(seed)
    gate = torch.sigmoid(torch.randn(N, C2, HW, generator=g))
    vn = 0.8 * torch.randn(N, C2, HW, generator=g) + 0.6
    bad = near(vn.double() - thresh, margin=2 * MARGIN)
    while bool(bad.any()):
        vn = torch.where(bad, 0.8 * torch.randn(N, C2, HW, generator=g) + 0.6, vn)
        bad = near(vn.double() - thresh, margin=2 * MARGIN)
    v = 0.7 * torch.randn(N, C2, HW, generator=g) + 0.3
    vsum = torch.randn(N, C2, HW, generator=g)
    grads = [torch.randn(N, C2, HW, generator=g) for _ in range(3)]          # g_v_out, g_vsum_out, g_spike
    return gate, vn, v, vsum, grads


def bwd_forward_inputs(gate, vn, v):
    """float64 (g_in, c_in) whose step forward reproduces the saved float32 gate and vn: g_in = logit(gate), c_in = vn - gate * v, with
    zero recurrent terms.  The comparison then measures the backward formula, not the rounding of a forward."""
    gd, vd = gate.double(), vn.double()
    return torch.log(gd) - torch.log1p(-gd), vd - gd * v.double()


def draw_tail(shape, Tm, Ts, seed):
    """v, vsum, spike_last, seg (0..Ts incl. Ts), t_last (-1 where seg == 0, else 0..Tm-2: a quiet element's last write is before the
    last step)"""
    g = _gen(seed)
    v = 0.7 * torch.randn(shape, generator=g) + 0.3
    vsum = torch.randn(shape, generator=g)
    spike_last = (torch.rand(shape, generator=g) < 0.4).float()
    seg = torch.randint(0, Ts + 1, shape, generator=g)
    tl = torch.randint(0, Tm - 1, shape, generator=g)
    tl = torch.where(seg == 0, torch.full_like(tl, -1), tl)
    return v, vsum, spike_last, seg.to(torch.int8), tl.to(torch.int8)


# group D: the whole chain through ops.arsnn_forward / ops.gated_recurrence with empty stacks
CHAIN_DIMS = (8, 3, 3, 9, 12)           # Tm, N, C2, H, W
CHAIN_CASES = [(ro, sat, wz, vr, Ts, (i % 3 == 0))
               for i, (ro, sat, wz, vr, Ts) in enumerate((ro, sat, wz, vr, Ts) for ro in ('sum', 'last', 'avg') for sat in (0, 1) for wz in (0, 1)
                                                         for vr in (None, 0.25) for Ts in (1, 3, 8))]        # ..., use_abs on every third
RUNNING_CASES = [(ro, relu, vr) for ro in ('sum', 'last') for relu in (False, True) for vr in (None, 0.25)]
CHAIN_SEED_OVERRIDES = {}               # case -> seed, where the default seed exceeds CAP_CHAIN


def chain_seed(case):
    return CHAIN_SEED_OVERRIDES.get(case, 100)


def draw_chain(seed, Ts_out):
    """X [Tm, N, 2*C2, H, W] (currents 0.8 * randn + 0.5: a fire rate near 0.37) and a gradient for the [Ts_out, N, C2, H, W] result"""
    Tm, N, C2, H, W = CHAIN_DIMS
    g = _gen(seed)
    X = torch.randn(Tm, N, 2 * C2, H, W, generator=g)
    X[:, :, C2:] = 0.8 * X[:, :, C2:] + 0.5
    G = torch.randn((Ts_out, N, C2, H, W) if Ts_out else (N, C2, H, W), generator=g)
    return X, G


# group E: the fused micro-step (second convolutions inside the launch)
FUSED_SHAPES = [(2, 16, 64), (1, 17, 68), (3, 5, 4), (800, 17, 4)]     # one tile | ragged 2 x 2 tiles | below a tile and the k = 7 halo | 1600 tiles > 256 * 6
FUSED_CASES = [(shape, k, rform, bias, prior) for shape in FUSED_SHAPES for k in (3, 5, 7) for rform in ('conv', 'const', 'zero')
               for bias in (True, False) for prior in (False, True)]
FUSED_SEED_OVERRIDES = {((3, 5, 4), 7, 'zero', True, True): 1000}               # case -> seed, where the default seed exceeds CAP_STEP


def fused_seed(case):
    return FUSED_SEED_OVERRIDES.get(case, 200 + FUSED_CASES.index(case))


def draw_fused(case):
    """-> dict of float32 CPU tensors: a_in, w_in, b_in | a_g, w_g, b_g | r_const | v, vsum (None where the case has none)"""
    (N, H, W), k, rform, bias, prior = case
    g = _gen(fused_seed(case))
    d = dict(a_in=torch.relu(torch.randn(N, 4, H, W, generator=g)), w_in=0.2 * torch.randn(4, 4, k, k, generator=g),
             b_in=torch.randn(4, generator=g) if bias else None, a_g=None, w_g=None, b_g=None, r_const=None, v=None, vsum=None)
    if rform == 'conv':
        d['a_g'] = torch.relu(torch.randn(N, 4, H, W, generator=g))
        d['w_g'] = 0.2 * torch.randn(4, 4, k, k, generator=g)
        d['b_g'] = torch.randn(4, generator=g) if bias else None
    elif rform == 'const':
        d['r_const'] = 0.5 * torch.randn(4, H, W, generator=g)
    if prior:
        d['v'] = 0.7 * torch.randn(N, 2, H, W, generator=g) + 0.3
        d['vsum'] = torch.randn(N, 2, H, W, generator=g)
    return d


def fused_conv_outputs(d):
    """float64 X = conv(a_in, w_in, b_in) and R (conv(a_g, w_g, b_g) | r_const | 0), each [N, 4, H, W]: for channel c2 the gate
    pre-activation is output c2, the current output 2 + c2"""
    F = torch.nn.functional
    k = d['w_in'].shape[-1]
    dbl = lambda a: None if a is None else a.double()
    X = F.conv2d(d['a_in'].double(), d['w_in'].double(), dbl(d['b_in']), padding=k // 2)
    if d['a_g'] is not None:
        R = F.conv2d(d['a_g'].double(), d['w_g'].double(), dbl(d['b_g']), padding=k // 2)
    elif d['r_const'] is not None:
        R = d['r_const'].double().unsqueeze(0).expand_as(X)
    else:
        R = torch.zeros_like(X)
    return X, R
