"""The adaptive sampler's step, tail and fused-step kernels (csrc/arsnn.hip) called directly through the C ABI, against the fp64
restatement of tests/sampler_ref.py differentiated by torch.autograd: random inputs, random CONSISTENT prior state (frozen elements with
seg == Ts included), agg pre-filled with random values (untouched slots must keep their bits), outputs pre-filled with NaN / 99.

Values: |got - ref| <= 1e-5 * (1 + |ref|).  Spikes: outside the margin |u| < 1e-4 (u = vn - thresh; also around the surrogate's box
edge) the bit must equal the reference's; inside it the reference is re-evaluated with the kernel's bit, so the element is still checked
for consistency.  The share of such elements is capped (tests/test_cpu_sampler_ref.py asserts the caps for the same seeds without a GPU).

Groups: A eas_arsnn_step_fwd | B eas_arsnn_step_bwd, eas_arsnn_tail_fwd / _bwd | C the grid-stride wraps | D the whole chain through
ops.arsnn_forward / ops.gated_recurrence with empty convolution stacks | E eas_arsnn_fused_step_fwd against fp64 convolutions + step."""
import pytest
import torch

import sampler_ref as sr

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -2          # include/eas_hip.h: EAS_ERR_INVALID_ARG, EAS_ERR_UNSUPPORTED
NAN = float('nan')
FP_OUTS = ('v_out', 'vsum_out', 'spike', 'gate', 'vn')
WORST, NEAR = {}, {}                       # per group: worst |got - ref| / (1 + |ref|), largest near-threshold share seen


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    yield torch.device('cuda:0')
    for g in sorted(WORST):
        print(f'\nsampler steps, group {g}: worst error {WORST[g]:.3g} (bar {sr.TOL:g}), largest near-threshold share {NEAR.get(g, 0.0):.3g}', end='')


def _close(got, ref, group, what):
    ref = ref.detach().to(got.device)
    assert got.shape == ref.shape, what
    if got.numel() == 0:
        return
    worst = float(((got.detach().double() - ref).abs() / (1 + ref.abs())).max())        # NaN (a sentinel left behind) fails the comparison
    WORST[group] = max(WORST.get(group, 0.0), worst) if worst == worst else NAN
    assert worst <= sr.TOL, f'{what}: worst |got - ref| / (1 + |ref|) = {worst:.3g}'


def _share(nr, cap, group, what):
    share = float(nr.double().mean())
    NEAR[group] = max(NEAR.get(group, 0.0), share)
    assert share <= cap, f'{what}: near-threshold share {share:.3g} above the cap {cap:g}'


def _reset_args(v_reset):
    return (0.0, 1) if v_reset is None else (float(v_reset), 0)


# ------------------------------------------------------------------------------------------------ launchers (sentinels in every output)
def _step_outs(shape, dev, saves=True):
    o = {n: torch.full(shape, NAN, device=dev) for n in (FP_OUTS if saves else FP_OUTS[:3])}
    for n in ('seg_b', 'tl_b'):
        o[n] = torch.full(shape, 99, dtype=torch.int8, device=dev) if saves else None
    o.setdefault('gate', None)
    o.setdefault('vn', None)
    return o


def _run_step_fwd(conv_in, conv_rec, v, vsum, seg, tl, agg, t, Ts, opt, thresh, saves=True, expect=0, outs=None):
    """eas_arsnn_step_fwd on clones of seg / tl / agg -> dict of everything it wrote"""
    from eas_snn_amd import _lib, ops
    ro, sat, vr = opt
    N, C2, HW = seg.shape
    o = _step_outs(seg.shape, seg.device, saves) if outs is None else outs
    o['seg'], o['tl'], o['agg'] = seg.clone(), tl.clone(), agg.clone()
    p = ops.ptr
    rc = _lib.lib().eas_arsnn_step_fwd(p(conv_in), p(conv_rec), p(v), p(vsum), p(o['seg']), p(o['tl']), p(o['agg']), p(o['v_out']),
                                       p(o['vsum_out']), p(o['spike']), p(o['gate']), p(o['vn']), p(o['seg_b']), p(o['tl_b']), t, Ts, ro,
                                       sat, thresh, *_reset_args(vr), N, C2, HW, ops.stream())
    assert rc == expect, f'eas_arsnn_step_fwd returned {rc}, expected {expect}'
    return o


def _run_fused_fwd(d, wr_in, wr_g, seg, tl, agg, t, Ts, opt, thresh, k, saves=True, expect=0, outs=None, W=None):
    """eas_arsnn_fused_step_fwd; d: the device tensors of sampler_ref.draw_fused; state tensors [N, 2, H, W]"""
    from eas_snn_amd import _lib, ops
    ro, sat, vr = opt
    N, _, H, Wt = seg.shape
    o = _step_outs(seg.shape, seg.device, saves) if outs is None else outs
    o['seg'], o['tl'], o['agg'] = seg.clone(), tl.clone(), agg.clone()
    p = ops.ptr
    rc = _lib.lib().eas_arsnn_fused_step_fwd(p(d['a_in']), p(wr_in), p(d['b_in']), p(d['a_g']), p(wr_g), p(d['b_g']), p(d['r_const']), p(d['v']),
                                             p(d['vsum']), p(o['seg']), p(o['tl']), p(o['agg']), p(o['v_out']), p(o['vsum_out']), p(o['spike']),
                                             p(o['gate']), p(o['vn']), p(o['seg_b']), p(o['tl_b']), t, Ts, ro, sat, thresh, *_reset_args(vr), N, H,
                                             Wt if W is None else W, k, ops.stream())
    assert rc == expect, f'eas_arsnn_fused_step_fwd returned {rc}, expected {expect}'
    return o


def _run_step_bwd(gv, gvs, gsp, g_agg, v_prev, vs_prev, gate, vn, seg_b, tl_b, t, Ts, opt, thresh):
    from eas_snn_amd import _lib, ops
    ro, sat, vr = opt
    N, C2, HW = gate.shape
    g_conv = torch.full((N, 2 * C2, HW), NAN, device=gate.device)
    g_vp, g_vsp = torch.full_like(gate, NAN), torch.full_like(gate, NAN)
    p = ops.ptr
    ops.check(_lib.lib().eas_arsnn_step_bwd(p(gv), p(gvs), p(gsp), p(g_agg), p(v_prev), p(vs_prev), p(gate), p(vn), p(seg_b), p(tl_b), p(g_conv),
                                            p(g_vp), p(g_vsp), t, Ts, ro, sat, thresh, *_reset_args(vr), 1.0, N, C2, HW, ops.stream()),
              'eas_arsnn_step_bwd')
    return g_conv, g_vp, g_vsp


def _run_tail(fn, *tensors_and_ints):
    from eas_snn_amd import _lib, ops
    args = [ops.ptr(a) if isinstance(a, torch.Tensor) else a for a in tensors_and_ints]
    ops.check(getattr(_lib.lib(), fn)(*args, ops.stream()), fn)


# ------------------------------------------------------------------------------------------------ the forward comparison (A, C, E)
def _check_step_fwd(o, g_in, c_in, g_rec, c_rec, v, vsum, seg0, tl0, agg0, t, Ts, opt, thresh, group, what, saves=True):
    """o: what the kernel wrote; g_in .. vsum: float64 inputs (v / vsum None = the first step); seg0 / tl0 / agg0: the state it started from"""
    ro, sat, vr = opt
    if v is None:
        v, vsum = torch.zeros_like(g_in), torch.zeros_like(g_in)
        seg0, tl0 = torch.zeros_like(seg0), torch.full_like(tl0, -1)
    seg64, tl64, agg64 = seg0.long(), tl0.long(), agg0.double()
    ref = sr.step(g_in, c_in, g_rec, c_rec, v, vsum, seg64, tl64, agg64, t, Ts, ro, sat, thresh, vr)
    nr = sr.near(ref[4] - thresh)
    _share(nr, sr.CAP_STEP, group, what)
    spike = o['spike'].double()
    assert torch.equal(spike[~nr], ref[2][~nr]), f'{what}: spike differs from the reference outside the margin'
    if not torch.equal(spike, ref[2]):        # inside the margin the rounding decides; everything else must follow the kernel's bit
        ref = sr.step(g_in, c_in, g_rec, c_rec, v, vsum, seg64, tl64, agg64, t, Ts, ro, sat, thresh, vr,
                      spike_override=torch.where(nr, spike, torch.full_like(spike, NAN)))
    v_out, vsum_out, sp, gate, vn, seg1, tl1, agg1 = ref
    assert torch.equal(spike, sp), what
    for name, want in (('v_out', v_out), ('vsum_out', vsum_out)) + ((('gate', gate), ('vn', vn)) if saves else ()):
        _close(o[name], want, group, f'{what}: {name}')
    assert torch.equal(o['seg'].long(), seg1) and torch.equal(o['tl'].long(), tl1), f'{what}: seg / t_last'
    if saves:
        assert torch.equal(o['seg_b'], seg0) and torch.equal(o['tl_b'], tl0), f'{what}: seg_before / t_last_before'
    hit = torch.zeros_like(agg0, dtype=torch.bool)
    if ro != 3:
        live = (sp != 0) & (seg64 < Ts)
        hit = live.unsqueeze(0) & (seg64.unsqueeze(0) == torch.arange(Ts, device=seg0.device).view((Ts,) + (1,) * seg0.dim()))
    assert torch.equal(o['agg'][~hit], agg0[~hit]), f'{what}: a slot of agg the step does not write changed'
    _close(o['agg'], agg1, group, f'{what}: agg')
    return int(hit.sum())


def _state(shape, t, Ts, seed, dev, **kw):
    g = sr._gen(seed)
    seg, tl = sr.draw_state(g, shape, t, Ts, **kw)
    agg = torch.randn((Ts,) + tuple(shape), generator=g)
    return seg.to(dev), tl.to(dev), agg.to(dev)


def _halves(conv, C2):
    return conv[:, :C2].double(), conv[:, C2:].double()


# ================================================================================================ group A
@pytest.mark.parametrize('t,Ts', sr.STEP_T_TS)
@pytest.mark.parametrize('shape', sr.STEP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_step_fwd_vs_fp64(dev, shape, t, Ts):
    """A1: every output, the new seg / t_last, seg_before / t_last_before and agg over the option grid at thresh 0.9
    (and thresh 1.0 once, on the first shape)"""
    N, C2, HW = shape
    written = 0
    for thresh in (sr.THRESH, 1.0) if (shape == sr.STEP_SHAPES[0] and (t, Ts) == (3, 3)) else (sr.THRESH,):
        conv_in, conv_rec, v, vsum = (a.to(dev) for a in sr.draw_step(shape, thresh))
        seg, tl, agg = _state(shape, t, Ts, 7 + t + 10 * Ts, dev)
        gi, ci = _halves(conv_in, C2)
        gr, cr = _halves(conv_rec, C2)
        for opt in sr.OPTIONS:
            o = _run_step_fwd(conv_in, conv_rec, v, vsum, seg, tl, agg, t, Ts, opt, thresh)
            written += _check_step_fwd(o, gi, ci, gr, cr, v.double(), vsum.double(), seg, tl, agg, t, Ts, opt, thresh, 'A',
                                       f'{shape} t={t} Ts={Ts} thresh={thresh:.1f} (readout, spike_attach, v_reset)={opt}')
    assert written > 0 or N * C2 * HW <= 4


@pytest.mark.parametrize('shape', sr.STEP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_step_fwd_first_step_null_state(dev, shape):
    """A2: v = vsum = NULL with garbage in seg / t_last equals the call with explicit zero state bit for bit; the four save
    pointers NULL leave the other outputs bit-identical"""
    N, C2, HW = shape
    Ts = 3
    conv_in, conv_rec, _, _ = (a.to(dev) for a in sr.draw_step(shape, sr.THRESH))
    g = sr._gen(5)
    garbage = [torch.randint(-128, 128, shape, generator=g).to(torch.int8).to(dev) for _ in range(2)]
    agg = torch.randn((Ts,) + tuple(shape), generator=g).to(dev)
    z = torch.zeros(shape, device=dev)
    seg0, tl0 = torch.zeros(shape, dtype=torch.int8, device=dev), torch.full(shape, -1, dtype=torch.int8, device=dev)
    gi, ci = _halves(conv_in, C2)
    gr, cr = _halves(conv_rec, C2)
    for opt in sr.OPTIONS:
        a = _run_step_fwd(conv_in, conv_rec, None, None, garbage[0], garbage[1], agg, 0, Ts, opt, sr.THRESH)
        b = _run_step_fwd(conv_in, conv_rec, z, z, seg0, tl0, agg, 0, Ts, opt, sr.THRESH)
        c = _run_step_fwd(conv_in, conv_rec, None, None, garbage[0], garbage[1], agg, 0, Ts, opt, sr.THRESH, saves=False)
        for n in a:
            assert torch.equal(a[n], b[n]), f'{opt}: {n} differs between NULL state and explicit zero state'
            assert c[n] is None or torch.equal(a[n], c[n]), f'{opt}: {n} differs when nothing is saved for the backward'
        _check_step_fwd(a, gi, ci, gr, cr, None, None, garbage[0], garbage[1], agg, 0, Ts, opt, sr.THRESH, 'A', f'{shape} first step {opt}')


def test_step_fwd_int8_limits(dev):
    """A3: Ts = 127, t = 126, counters at 125 / 126 / 127 (frozen), last writes at 124 / 125: the sign handling of the packed bytes"""
    shape, t, Ts = (1, 1, 64), 126, 127
    conv_in, conv_rec, v, vsum = (a.to(dev) for a in sr.draw_step(shape, sr.THRESH))
    seg, tl, agg = _state(shape, t, Ts, 9, dev, seg_values=[0, 1, 125, 126, 127], tl_values=[-1, 0, 124, 125])
    assert set(seg.flatten().tolist()) == {0, 1, 125, 126, 127} and {0, 124, 125} <= set(tl.flatten().tolist())
    tl = torch.where((seg > 0) & (tl < 0), torch.zeros_like(tl), tl)          # t_last = -1 exactly where seg == 0
    gi, ci = _halves(conv_in, 1)
    gr, cr = _halves(conv_rec, 1)
    for opt in sr.OPTIONS:
        o = _run_step_fwd(conv_in, conv_rec, v, vsum, seg, tl, agg, t, Ts, opt, sr.THRESH)
        _check_step_fwd(o, gi, ci, gr, cr, v.double(), vsum.double(), seg, tl, agg, t, Ts, opt, sr.THRESH, 'A', f'int8 limits {opt}')


def _untouched(o, seg, tl, agg, what):
    for n in FP_OUTS:
        assert bool(torch.isnan(o[n]).all()), f'{what}: {n} was written'
    assert bool((o['seg_b'] == 99).all()) and bool((o['tl_b'] == 99).all()), f'{what}: saved state was written'
    assert torch.equal(o['seg'], seg) and torch.equal(o['tl'], tl) and torch.equal(o['agg'], agg), f'{what}: state was written'


def test_refusals_are_decided_before_any_launch(dev):
    """A4: unsupported sizes and invalid arguments come back as a status and leave every sentinel in place.  Every buffer is large
    enough for the refused geometry, so nothing here can touch memory it does not own."""
    from eas_snn_amd import _lib, ops
    opt = (0, 1, 0.25)
    g = sr._gen(2)
    N, C2, HW, TsMax = 2, 2, 8, 128
    shape = (N, C2, HW)
    conv_in, conv_rec = torch.randn(N, 2 * C2, HW, generator=g).to(dev), torch.randn(N, 2 * C2, HW, generator=g).to(dev)
    v, vsum = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    seg, tl = torch.zeros(shape, dtype=torch.int8, device=dev), torch.full(shape, -1, dtype=torch.int8, device=dev)
    agg = torch.randn((TsMax,) + shape, generator=g).to(dev)
    run = lambda **kw: _run_step_fwd(conv_in, conv_rec, kw.pop('v', v), kw.pop('vsum', vsum), kw.pop('seg', seg), tl, agg, kw.pop('t', 3),
                                     kw.pop('Ts', 3), kw.pop('opt', opt), sr.THRESH, **kw)
    _untouched(run(Ts=128, expect=E_UNSUPPORTED), seg, tl, agg, 'Ts = 128')
    _untouched(run(t=127, expect=E_UNSUPPORTED), seg, tl, agg, 't = 127')
    _untouched(run(seg=seg[:, :, :6].contiguous(), expect=E_UNSUPPORTED), seg[:, :, :6], tl, agg, 'HW = 6')
    _untouched(run(vsum=None, expect=E_INVALID), seg, tl, agg, 'v without vsum')
    _untouched(run(opt=(4, 1, 0.25), expect=E_INVALID), seg, tl, agg, 'readout = 4')
    outs = _step_outs(shape, dev)
    longer = torch.full((N * C2 * HW + 4,), NAN, device=dev)
    outs['v_out'] = longer[1:1 + N * C2 * HW].view(shape)
    _untouched(run(outs=outs, expect=E_INVALID), seg, tl, agg, 'v_out off by one float')
    assert bool(torch.isnan(longer).all())
    # the fused step: the same checks, and W % 4 and the kernel size
    H, W, k = 2, 8, 3
    fshape = (N, 2, H, W)
    d = dict(a_in=torch.randn(N, 4, H, W, generator=g).to(dev), b_in=None, a_g=None, b_g=None, r_const=None,
             v=torch.randn(fshape, generator=g).to(dev), vsum=torch.randn(fshape, generator=g).to(dev))
    wr = torch.randn(_lib.lib().eas_smallconv_packed_floats(4, 7, 4), generator=g).to(dev)          # room for k = 7
    fseg, ftl = torch.zeros(fshape, dtype=torch.int8, device=dev), torch.full(fshape, -1, dtype=torch.int8, device=dev)
    fagg = torch.randn((TsMax,) + fshape, generator=g).to(dev)
    frun = lambda dd=d, **kw: _run_fused_fwd(dd, wr, None, fseg, ftl, fagg, kw.pop('t', 3), kw.pop('Ts', 3), kw.pop('opt', opt), sr.THRESH,
                                             kw.pop('k', k), **kw)
    _untouched(frun(Ts=128, expect=E_UNSUPPORTED), fseg, ftl, fagg, 'fused Ts = 128')
    _untouched(frun(t=127, expect=E_UNSUPPORTED), fseg, ftl, fagg, 'fused t = 127')
    _untouched(frun(W=6, expect=E_UNSUPPORTED), fseg, ftl, fagg, 'fused W = 6')
    _untouched(frun(k=4, expect=E_UNSUPPORTED), fseg, ftl, fagg, 'fused k = 4')
    _untouched(frun(dict(d, vsum=None), expect=E_INVALID), fseg, ftl, fagg, 'fused v without vsum')
    _untouched(frun(opt=(4, 1, 0.25), expect=E_INVALID), fseg, ftl, fagg, 'fused readout = 4')
    outs = _step_outs(fshape, dev)
    longer = torch.full((N * 2 * H * W + 4,), NAN, device=dev)
    outs['v_out'] = longer[1:1 + N * 2 * H * W].view(fshape)
    _untouched(frun(outs=outs, expect=E_INVALID), fseg, ftl, fagg, 'fused v_out off by one float')
    assert bool(torch.isnan(longer).all())
    # the tails have no readout 3
    L, p, spike = _lib.lib(), ops.ptr, torch.zeros(shape, device=dev)
    a2, gv, gvs = agg.clone(), torch.full(shape, NAN, device=dev), torch.full(shape, NAN, device=dev)
    assert L.eas_arsnn_tail_fwd(p(v), p(vsum), p(spike), p(seg), p(tl), p(a2), 4, 3, 3, 0, N, C2, HW, ops.stream()) == E_INVALID
    assert L.eas_arsnn_tail_bwd(p(agg), p(spike), p(seg), p(tl), p(gv), p(gvs), 4, 3, 3, 0, N, C2, HW, ops.stream()) == E_INVALID
    assert torch.equal(a2, agg) and bool(torch.isnan(gv).all()) and bool(torch.isnan(gvs).all())


# ================================================================================================ group B
def _ref_step_bwd(gate, vn, v, vsum, seg_b, tl_b, grads, g_agg, t, Ts, opt, thresh):
    """autograd of sampler_ref.step at the saved float32 gate / vn -> (g_gatepre, g_cur, g_v_prev, g_vsum_prev), float64"""
    ro, sat, vr = opt
    g_in, c_in = sr.bwd_forward_inputs(gate, vn, v)
    leaves = [a.requires_grad_(True) for a in (g_in, c_in, v.double(), vsum.double())]
    z = torch.zeros_like(g_in)
    out = sr.step(leaves[0], leaves[1], z, z, leaves[2], leaves[3], seg_b.long(), tl_b.long(), torch.zeros_like(g_agg, dtype=torch.float64), t, Ts,
                  ro, sat, thresh, vr)
    assert float((out[4].detach() - vn.double()).abs().max()) < 1e-12 and float((out[3].detach() - gate.double()).abs().max()) < 1e-12
    assert not bool(sr.near(out[4] - thresh).any())                    # group B: no element near a threshold, by construction
    loss = sum((g.double() * o).sum() for g, o in zip(grads, out[:3])) + (g_agg.double() * out[7]).sum()
    got = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [torch.zeros_like(z) if a is None else a for a in got]


def _bwd_case(shape, t, Ts, thresh, dev, seed=sr.BWD_SEED):
    gate, vn, v, vsum, grads = sr.draw_bwd(shape, thresh, seed)
    g = sr._gen(seed + 1000 + t + 10 * Ts)
    seg_b, tl_b = sr.draw_state(g, shape, t, Ts)
    g_agg = torch.randn((Ts,) + tuple(shape), generator=g)
    return [a.to(dev) for a in (gate, vn, v, vsum)], [a.to(dev) for a in grads], seg_b.to(dev), tl_b.to(dev), g_agg.to(dev)


def _check_step_bwd(got, want, C2, group, what):
    g_conv, g_vp, g_vsp = got
    _close(g_conv[:, :C2], want[0], group, f'{what}: g_conv, gate half')
    _close(g_conv[:, C2:], want[1], group, f'{what}: g_conv, current half')
    _close(g_vp, want[2], group, f'{what}: g_v_prev')
    _close(g_vsp, want[3], group, f'{what}: g_vsum_prev')


@pytest.mark.parametrize('t,Ts', sr.STEP_T_TS)
@pytest.mark.parametrize('shape', sr.STEP_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_step_bwd_vs_autograd_of_fp64(dev, shape, t, Ts):
    """B1: g_conv (both halves), g_v_prev, g_vsum_prev against torch.autograd of the reference step, over the option grid"""
    for thresh in (sr.THRESH, 1.0) if (shape == sr.STEP_SHAPES[0] and (t, Ts) == (3, 3)) else (sr.THRESH,):
        (gate, vn, v, vsum), grads, seg_b, tl_b, g_agg = _bwd_case(shape, t, Ts, thresh, dev)
        for opt in sr.OPTIONS:
            got = _run_step_bwd(*grads, g_agg, v, vsum, gate, vn, seg_b, tl_b, t, Ts, opt, thresh)
            want = _ref_step_bwd(gate, vn, v, vsum, seg_b, tl_b, grads, g_agg, t, Ts, opt, thresh)
            _check_step_bwd(got, want, shape[1], 'B', f'{shape} t={t} Ts={Ts} thresh={thresh:.1f} (readout, spike_attach, v_reset)={opt}')


def test_step_bwd_null_forms(dev):
    """B2: a NULL incoming gradient equals a zero tensor, NULL v_prev / vsum_prev equal zero tensors, bit for bit"""
    shape, t, Ts = sr.STEP_SHAPES[0], 3, 3
    (gate, vn, v, vsum), grads, seg_b, tl_b, g_agg = _bwd_case(shape, t, Ts, sr.THRESH, dev)
    z = torch.zeros(shape, device=dev)
    for opt in sr.OPTIONS:
        for i in range(3):
            with_null = _run_step_bwd(*[None if j == i else g for j, g in enumerate(grads)], g_agg, v, vsum, gate, vn, seg_b, tl_b, t, Ts, opt, sr.THRESH)
            with_zero = _run_step_bwd(*[z if j == i else g for j, g in enumerate(grads)], g_agg, v, vsum, gate, vn, seg_b, tl_b, t, Ts, opt, sr.THRESH)
            assert all(torch.equal(a, b) and not bool(torch.isnan(a).any()) for a, b in zip(with_null, with_zero)), f'{opt}: gradient {i} NULL vs zero'
        with_null = _run_step_bwd(*grads, g_agg, None, None, gate, vn, seg_b, tl_b, t, Ts, opt, sr.THRESH)
        with_zero = _run_step_bwd(*grads, g_agg, z, z, gate, vn, seg_b, tl_b, t, Ts, opt, sr.THRESH)
        assert all(torch.equal(a, b) and not bool(torch.isnan(a).any()) for a, b in zip(with_null, with_zero)), f'{opt}: v_prev NULL vs zero'


def _check_tail(shape, Tm, Ts, ro, wz, dev, group, seed=31):
    N, C2, HW = shape
    v, vsum, spike_last, seg, tl = (a.to(dev) for a in sr.draw_tail(shape, Tm, Ts, seed))
    g = sr._gen(seed + 1)
    agg0 = torch.randn((Ts,) + tuple(shape), generator=g).to(dev)
    g_agg = torch.randn((Ts,) + tuple(shape), generator=g).to(dev)
    what = f'tail {shape} Ts={Ts} readout={ro} write_zero={wz}'
    quiet_free = (spike_last == 0) & (seg < Ts)
    assert bool((seg == Ts).any()) and bool((spike_last == 1).any()) and bool((quiet_free & (tl == -1)).any()), what
    agg = agg0.clone()
    _run_tail('eas_arsnn_tail_fwd', v, vsum, spike_last, seg, tl, agg, Tm, Ts, ro, wz, N, C2, HW)
    v64, vs64 = v.double().requires_grad_(True), vsum.double().requires_grad_(True)
    ref = sr.tail(v64, vs64, spike_last.double(), seg.long(), tl.long(), agg0.double(), Tm, Ts, ro, wz)
    hit = quiet_free.unsqueeze(0) & (seg.long().unsqueeze(0) == torch.arange(Ts, device=dev).view(Ts, 1, 1, 1))
    assert torch.equal(agg[~hit], agg0[~hit]), f'{what}: a slot of agg the tail does not write changed'
    _close(agg, ref, group, f'{what}: agg')
    g_v, g_vs = torch.full(shape, NAN, device=dev), torch.full(shape, NAN, device=dev)
    _run_tail('eas_arsnn_tail_bwd', g_agg, spike_last, seg, tl, g_v, g_vs, Tm, Ts, ro, wz, N, C2, HW)
    want = torch.autograd.grad((g_agg.double() * ref).sum(), [v64, vs64], allow_unused=True)
    want = [torch.zeros_like(v64) if a is None else a for a in want]
    _close(g_v, want[0], group, f'{what}: g_v')
    _close(g_vs, want[1], group, f'{what}: g_vsum')
    if wz:
        assert bool((g_v == 0).all()) and bool((g_vs == 0).all()), f'{what}: a gradient through a segment written as zero'
    else:
        assert bool((g_v != 0).any() or (g_vs != 0).any()), what


@pytest.mark.parametrize('Ts', [1, 3])
@pytest.mark.parametrize('wz', [0, 1])
@pytest.mark.parametrize('ro', [0, 1, 2])
def test_tail_fwd_bwd_vs_fp64(dev, ro, wz, Ts):
    """B3: frozen elements (seg == Ts), elements that fired in the last step, elements that never wrote (t_last = -1, divisor Tm)"""
    _check_tail(sr.STEP_SHAPES[0], 6, Ts, ro, wz, dev, 'B')


# ================================================================================================ group C
def test_step_grid_stride_wrap(dev):
    """C1: N * C2 * HW just above 8192 blocks x 256 threads x 4 elements: the forward's grid-stride loop wraps (the backward's, one
    element per thread, wraps at a quarter of this)"""
    shape, t, Ts, opt = sr.WRAP_SHAPE, 1, 2, (0, 1, 0.25)
    N, C2, HW = shape
    assert N * C2 * HW > 8192 * 256 * 4
    conv_in, conv_rec, v, vsum = (a.to(dev) for a in sr.draw_step(shape, sr.THRESH))
    seg, tl, agg = _state(shape, t, Ts, 17, dev)
    o = _run_step_fwd(conv_in, conv_rec, v, vsum, seg, tl, agg, t, Ts, opt, sr.THRESH)
    gi, ci = _halves(conv_in, C2)
    gr, cr = _halves(conv_rec, C2)
    _check_step_fwd(o, gi, ci, gr, cr, v.double(), vsum.double(), seg, tl, agg, t, Ts, opt, sr.THRESH, 'C', 'wrap forward')
    del o, conv_in, conv_rec, gi, ci, gr, cr
    (gate, vn, v, vsum), grads, seg_b, tl_b, g_agg = _bwd_case(shape, t, Ts, sr.THRESH, dev)
    got = _run_step_bwd(*grads, g_agg, v, vsum, gate, vn, seg_b, tl_b, t, Ts, opt, sr.THRESH)
    want = _ref_step_bwd(gate, vn, v, vsum, seg_b, tl_b, grads, g_agg, t, Ts, opt, sr.THRESH)
    _check_step_bwd(got, want, C2, 'C', 'wrap backward')


def test_tail_grid_stride_wrap(dev):
    """C2: both tail kernels at the same size"""
    _check_tail(sr.WRAP_SHAPE, 2, 2, 0, 0, dev, 'C')


# ================================================================================================ group D
def _element_mask_on_grad(g, C2):
    """[Tm, N, 2*C2, H, W] -> [Tm, 2, N, C2, H, W]: both gradient entries of an element (n, c, h, w) side by side"""
    Tm, N, _, H, W = g.shape
    return g.reshape(Tm, N, 2, C2, H, W).permute(0, 2, 1, 3, 4, 5)


@pytest.mark.parametrize('case', sr.CHAIN_CASES, ids=lambda c: '-'.join(str(x) for x in c))
def test_chain_with_empty_stacks_vs_fp64(dev, case):
    """D1: ops.arsnn_forward with EMPTY input and gate stacks = eas_arsnn_step_fwd x Tm, the tail, the ReLU and the whole backward chain
    with no convolution, so a rounding flip stays inside its own element.  Elements whose fp64 trajectory is near a threshold at any
    step are left out with all their output slots and gradient entries; everything else must match."""
    from eas_snn_amd import ops
    ro, sat, wz, vr, Ts, ab = case
    Tm, N, C2, H, W = sr.CHAIN_DIMS
    X, G = sr.draw_chain(sr.chain_seed(case), Ts)
    Xd, G = X.to(dev).requires_grad_(True), G.to(dev)
    out, _ = ops.arsnn_forward(Xd, [], [], 5, Ts, ro, bool(sat), bool(wz), ab, sr.THRESH, vr)
    out.backward(G)
    X64 = X.double().to(dev).requires_grad_(True)
    want, u = sr.chain(X64, Ts, ro, sat, wz, ab, sr.THRESH, vr)
    want_g, = torch.autograd.grad((want * G.double()).sum(), X64)
    bad = sr.near(u).any(0)
    _share(bad, sr.CAP_CHAIN, 'D', str(case))
    keep = ~bad
    assert out.shape == want.shape and Xd.grad.shape == X.shape
    _close(out[:, keep], want[:, keep], 'D', f'{case}: output')
    _close(_element_mask_on_grad(Xd.grad, C2)[:, :, keep], _element_mask_on_grad(want_g, C2)[:, :, keep], 'D', f'{case}: input gradient')
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(Xd.grad).any())


@pytest.mark.parametrize('case', sr.RUNNING_CASES, ids=lambda c: '-'.join(str(x) for x in c))
def test_gated_recurrence_with_empty_stacks_vs_fp64(dev, case):
    """D2: readout 3 (the running sum / the last potential), forward and backward, through ops.gated_recurrence"""
    from eas_snn_amd import ops
    ro, relu, vr = case
    Tm, N, C2, H, W = sr.CHAIN_DIMS
    X, G = sr.draw_chain(sr.chain_seed(case), 0)
    Xd, G = X.to(dev).requires_grad_(True), G.to(dev)
    out = ops.gated_recurrence(Xd, [], [], 5, ro, relu, sr.THRESH, vr)
    out.backward(G)
    X64 = X.double().to(dev).requires_grad_(True)
    want, u = sr.chain(X64, 1, 0, 0, 0, relu, sr.THRESH, vr, running=ro)
    want_g, = torch.autograd.grad((want * G.double()).sum(), X64)
    bad = sr.near(u).any(0)
    _share(bad, sr.CAP_CHAIN, 'D', str(case))
    keep = ~bad
    _close(out[keep], want[keep], 'D', f'{case}: output')
    _close(_element_mask_on_grad(Xd.grad, C2)[:, :, keep], _element_mask_on_grad(want_g, C2)[:, :, keep], 'D', f'{case}: input gradient')


# ================================================================================================ group E
@pytest.mark.parametrize('case', sr.FUSED_CASES, ids=lambda c: f'{c[0][0]}x{c[0][1]}x{c[0][2]}-k{c[1]}-{c[2]}-b{int(c[3])}-p{int(c[4])}')
def test_fused_step_vs_fp64_convolutions_plus_step(dev, case):
    """E: the fused micro-step against fp64 convolutions on the CPU followed by the reference step, over the option grid: one tile,
    ragged tiles, a map below a tile and the k = 7 halo, and more tiles than blocks (the tile loop wraps); the gate stack's part from a
    convolution, from one shared image, or absent; biases given or NULL; first step (v = NULL, garbage counters) or a random state"""
    from eas_snn_amd import ops
    (N, H, W), k, rform, bias, prior = case
    shape = (N, 2, H, W)
    cpu = sr.draw_fused(case)
    X, R = (a.to(dev) for a in sr.fused_conv_outputs(cpu))
    d = {n: None if a is None else a.to(dev) for n, a in cpu.items()}
    wr_in = ops.smallconv_pack([(d['w_in'], 0, 4, 0, None)])[0]
    wr_g = ops.smallconv_pack([(d['w_g'], 0, 4, 0, None)])[0] if rform == 'conv' else None
    t, Ts = (3, 3) if prior else (0, 1 if bias else 3)
    g = sr._gen(sr.fused_seed(case) + 5000)
    if prior:
        seg, tl = sr.draw_state(g, shape, t, Ts)
    else:
        seg, tl = (torch.randint(-128, 128, shape, generator=g).to(torch.int8) for _ in range(2))
    seg, tl, agg = seg.to(dev), tl.to(dev), torch.randn((Ts,) + shape, generator=g).to(dev)
    v64, vs64 = (d['v'].double(), d['vsum'].double()) if prior else (None, None)
    for opt in sr.OPTIONS:
        o = _run_fused_fwd(d, wr_in, wr_g, seg, tl, agg, t, Ts, opt, sr.THRESH, k)
        _check_step_fwd(o, X[:, :2], X[:, 2:], R[:, :2], R[:, 2:], v64, vs64, seg, tl, agg, t, Ts, opt, sr.THRESH, 'E', f'{case} {opt}')
