"""tests/sampler_ref.py without a GPU: (1) stepped through the oracle's own convolutions in float32 it equals
oracle.embedding_ref.AdaptiveRSNNEmbeddingRef -- which the goldens pin to the reference project -- in output and input gradient;
(2) for every seed and shape tests/test_gpu_sampler_steps.py uses, the share of near-threshold elements of the fp64 reference alone
stays within the cap the device comparison allows (a condition on the inputs, checked where no kernel is involved)."""
import itertools

import pytest
import torch

import sampler_ref as sr
from oracle.embedding_ref import AdaptiveRSNNEmbeddingRef, _to_time_major_reversed


def _stepwise(m, events, G):
    """the module's convolutions, the reference's step / tail"""
    ev = _to_time_major_reversed(events)
    Tm = ev.shape[0]
    z = torch.zeros_like(ev[0])
    v, vsum, spike = z, z, z
    seg = torch.zeros(z.shape, dtype=torch.int64)
    t_last = torch.full_like(seg, -1)
    agg = torch.zeros((m.Ts,) + z.shape)
    for t in range(Tm):
        g_rec, c_rec = m.gate_conv(spike).chunk(2, dim=-3)
        g_in, c_in = m.input_conv(ev[t]).chunk(2, dim=-3)
        v, vsum, spike, _, _, seg, t_last, agg = sr.step(g_in, c_in, g_rec, c_rec, v, vsum, seg, t_last, agg, t, m.Ts, m.readout,
                                                         m.spike_attach, m.thresh, m.vreset)
    out = sr.tail(v, vsum, spike, seg, t_last, agg, Tm, m.Ts, m.readout, m.write_zero)
    if m.abs:
        out = torch.relu(out)
    g, = torch.autograd.grad((out * G).sum(), events)
    return out.detach(), g


@pytest.mark.parametrize('depth', [1, 2])
@pytest.mark.parametrize('Ts', [1, 3])
def test_reference_equals_the_oracle(depth, Ts):
    B, Tm, H, W = 2, 5, 6, 8
    fired_any = frozen_any = False
    for i, (readout, sat, wz, ab, vreset) in enumerate(itertools.product(('sum', 'last', 'avg'), (False, True), (False, True),
                                                                         (False, True), (None, 0.0))):
        torch.manual_seed(1000 * depth + 100 * Ts + i)
        m = AdaptiveRSNNEmbeddingRef(3, Ts=Ts, spike_attach=sat, write_zero=wz, abs=ab, depth=depth, readout=readout, Tm=Tm,
                                     thresh=1.0, vreset=vreset)
        events = torch.poisson(torch.full((B, Tm, 2, H, W), 0.7)).requires_grad_(True)
        G = torch.randn(Ts, B, 2, H, W)
        want, rec = m(events, record=True)
        want_g, = torch.autograd.grad((want * G).sum(), events)
        got, got_g = _stepwise(m, events, G)
        what = f'{readout} sat={sat} wz={wz} abs={ab} vreset={vreset}'
        torch.testing.assert_close(got, want.detach(), rtol=1e-6, atol=1e-6, msg=lambda s: f'{what}: {s}')
        torch.testing.assert_close(got_g, want_g, rtol=1e-6, atol=1e-6, msg=lambda s: f'{what}: {s}')
        fired_any |= bool((rec[-1] >= 0).any())
        frozen_any |= Ts == 1 and bool((rec[-1] >= 0).float().mean() > 0.1)
    assert fired_any and (Ts != 1 or frozen_any)          # the comparison saw segment writes, and elements past their Ts segments


def test_spike_override_replaces_the_forward_value_only():
    g = torch.Generator().manual_seed(3)
    shape = (2, 3, 8)
    gi, ci, v, vs = (torch.randn(shape, dtype=torch.float64, generator=g).requires_grad_(True) for _ in range(4))
    z = torch.zeros(shape, dtype=torch.float64)
    seg, tl = torch.zeros(shape, dtype=torch.int64), torch.full(shape, -1)
    agg = torch.zeros((2,) + shape, dtype=torch.float64)
    base = sr.step(gi, ci, z, z, v, vs, seg, tl, agg, 0, 2, 0, 1, 0.3, 0.25)
    flip = torch.full(shape, float('nan'), dtype=torch.float64)
    flip[0, 0, :4] = 1 - base[2].detach()[0, 0, :4]
    got = sr.step(gi, ci, z, z, v, vs, seg, tl, agg, 0, 2, 0, 1, 0.3, 0.25, spike_override=flip)
    assert torch.equal(got[2][0, 0, :4], flip[0, 0, :4]) and torch.equal(got[2][1], base[2][1])
    assert torch.equal(got[5][0, 0, :4], flip[0, 0, :4].long())          # the segment counter follows the forced spike
    # the forced spike still carries the surrogate's gradient
    ga, = torch.autograd.grad(got[2].sum(), ci)
    gb, = torch.autograd.grad(base[2].sum(), ci)
    assert torch.equal(ga, gb)
    keep = torch.full(shape, float('nan'), dtype=torch.float64)
    same = sr.step(gi, ci, z, z, v, vs, seg, tl, agg, 0, 2, 0, 1, 0.3, 0.25, spike_override=keep)
    assert all(torch.equal(a, b) for a, b in zip(same, base))


# ------------------------------------------------------------------------------------------------ the caps, for the reference alone
def _share(u):
    return float(sr.near(u).double().mean())


@pytest.mark.parametrize('key', list(sr.STEP_SEEDS), ids=lambda k: f'{k[0][0]}x{k[0][1]}x{k[0][2]}-{k[1]:.1f}')
def test_cap_step_inputs(key):
    """groups A and C1: one step from a random prior state, and the same currents as a first step (v = NULL)"""
    shape, thresh = key
    conv_in, conv_rec, v, _ = sr.draw_step(shape, thresh)
    assert _share(sr.step_u(conv_in, conv_rec, v, thresh)) <= sr.CAP_STEP
    assert _share(sr.step_u(conv_in, conv_rec, None, thresh)) <= sr.CAP_STEP


@pytest.mark.parametrize('shape', sr.STEP_SHAPES + [sr.WRAP_SHAPE], ids=str)
def test_cap_backward_inputs_have_no_near_element(shape):
    """groups B and C1: the drawn vn, and the vn the fp64 forward rebuilds from (g_in, c_in), are outside every margin"""
    for thresh in (sr.THRESH, 1.0):
        gate, vn, v, _, _ = sr.draw_bwd(shape, thresh)
        g_in, c_in = sr.bwd_forward_inputs(gate, vn, v)
        vn64 = torch.sigmoid(g_in) * v.double() + c_in
        assert _share(vn.double() - thresh) == sr.CAP_BWD and _share(vn64 - thresh) == sr.CAP_BWD
        assert float((vn64 - vn.double()).abs().max()) < 1e-12 and float((torch.sigmoid(g_in) - gate.double()).abs().max()) < 1e-12


@pytest.mark.parametrize('case', sr.CHAIN_CASES, ids=lambda c: '-'.join(str(x) for x in c))
def test_cap_chain(case):
    """group D1: elements whose trajectory is near a threshold at ANY of the Tm steps"""
    ro, sat, wz, vr, Ts, ab = case
    X, _ = sr.draw_chain(sr.chain_seed(case), Ts)
    _, u = sr.chain(X.double(), Ts, ro, sat, wz, ab, sr.THRESH, vr)
    assert float(sr.near(u).any(0).double().mean()) <= sr.CAP_CHAIN


@pytest.mark.parametrize('case', sr.RUNNING_CASES, ids=lambda c: '-'.join(str(x) for x in c))
def test_cap_running(case):
    """group D2"""
    ro, relu, vr = case
    X, _ = sr.draw_chain(sr.chain_seed(case), 0)
    _, u = sr.chain(X.double(), 1, 0, 0, 0, relu, sr.THRESH, vr, running=ro)
    assert float(sr.near(u).any(0).double().mean()) <= sr.CAP_CHAIN


def test_chain_draw_populates_every_branch():
    """the D inputs: a fire rate near 0.37, more than half the elements reach three segments"""
    X, _ = sr.draw_chain(100, 3)
    for vr in (None, 0.25):
        _, u = sr.chain(X.double(), 8, 'sum', 0, 0, 0, sr.THRESH, vr)
        fires = (u > 0).sum(0)
        assert 0.25 < float((u > 0).double().mean()) < 0.5 and float((fires >= 3).double().mean()) > 0.5


@pytest.mark.parametrize('case', sr.FUSED_CASES, ids=lambda c: f'{c[0][0]}x{c[0][1]}x{c[0][2]}-k{c[1]}-{c[2]}-b{int(c[3])}-p{int(c[4])}')
def test_cap_fused(case):
    """group E"""
    d = sr.draw_fused(case)
    X, R = sr.fused_conv_outputs(d)
    assert _share(sr.step_u(X, R, d['v'], sr.THRESH)) <= sr.CAP_STEP
