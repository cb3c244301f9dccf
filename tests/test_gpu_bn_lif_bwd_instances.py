"""eas_bn_lif_bwd: every instance of the backward's table (bn_lif.hip kBwdInstances) against the CPU oracle.

The backward picks, per call, a kernel instance from one table: a FAST instance (surrogate and reset form compiled in, plain operands) where
the table has one for the call, the GENERIC instance (everything decided from the launch arguments) otherwise.  This file calls the C ABI
directly so that every operand form reaches every instance:

  * yardstick: ``oracle/sj_ref`` neuron + torch BatchNorm in fp64 on the CPU, with the tolerances of
    ``test_gpu_kernels.py::test_bn_lif_fused_vs_oracle`` (grad_y rtol 2e-3 / atol 2e-5, BatchNorm parameter gradients rtol 2e-3 / atol 2e-4,
    scalar gradients rtol 2e-3 / atol 1e-4; a neuron whose spike train flipped at the threshold is left out elementwise and gives the sums
    one neuron's worth of slack, as there).  dL/dalpha of the learnable slope is a scalar reduced like dL/dw and gets dL/dw's tolerance.
  * shapes: the smallest that reach each path.  Two passes: C = 9 (not a multiple of the 8-wide channel grid) at HW = 8 and 12; one pass
    (one block per channel, C >= 64): HW = 8 (256-thread blocks, most threads idle) and the first size past 256 * GPT groups (512-thread
    blocks, ragged last groups).
  * operands: plain, + grad_mean, + v_init, channel slices (grad_s / y / grad_y inside wider tensors; the rest of the wide grad_y must stay
    untouched), a broadcast input frame, and running statistics with inputs that sit EXACTLY on the threshold (dyadic values: fp32 and fp64
    then agree bit for bit, spikes included).
  * extra (not the yardstick): where the table has a fast instance, EAS_BNLIF_BWD=generic must give the same bits, and the kernel trace must
    show the instance the table promises."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SG = {'atan': 0, 'sigmoid': 1, 'rect': 2, 'patan': 3}
ALPHA = {'atan': 2.0, 'sigmoid': 4.0, 'rect': 1.0, 'patan': 1.5}
FLAG_HARD, FLAG_DETACH = 1, 4
# what bn_lif.hip builds fast instances for: soft reset, decay_input = False, attached reset, ATan, T in {3, 5, 7}; two-pass form: plain operands
FAST_T = (3, 5, 7)
PLAIN_VARIANTS = ('plain', 'slices', 'threshold')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


class _RectFn(torch.autograd.Function):
    """box surrogate of width 1/alpha and height alpha around the threshold, firing at u >= 0 like the fused layer"""

    @staticmethod
    def forward(ctx, u, alpha):
        ctx.save_for_backward(u)
        ctx.alpha = alpha
        return (u >= 0).to(u.dtype)

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        return torch.where(u.abs() < 0.5 / ctx.alpha, g * ctx.alpha, torch.zeros_like(g)), None


def _oracle_surrogate(sg):
    from oracle import sj_ref
    if sg == 'atan':
        return sj_ref.ATan(ALPHA[sg])
    if sg == 'sigmoid':
        return sj_ref.Sigmoid(ALPHA[sg])
    if sg == 'patan':
        return sj_ref.PATan(ALPHA[sg]).double().train()
    return lambda u: _RectFn.apply(u, ALPHA[sg])


def _one_pass_512_hw(T):
    gpt = 3 if T <= 3 else (2 if T <= 5 else 1)
    return 4 * (128 * gpt + 2)          # N = 2: 256 * GPT + 4 groups, the first even count past the 256-thread form


def _inputs(T, N, C, HW, variant, seed, v0=0.0):
    """numpy inputs of one call.  'threshold': dyadic values and identity statistics, so that many potentials land exactly on v_th"""
    rng = np.random.default_rng(seed)
    H, W = 2, HW // 2
    d = {}
    if variant == 'threshold':
        d['y'] = (rng.integers(-4, 9, (T, N, C, H, W)) * 0.25).astype(np.float32)       # multiples of 1/4 in [-1, 2]: h = v / 2 + y is exact
        d['y'][0, :, :, 0, 0] = 1.0 - v0                                                 # h = v0 + y = 1 = v_th at the first step
        d['g_s'] = (rng.integers(-8, 9, (T, N, C, H, W)) * 0.125).astype(np.float32)
        d['gamma'], d['beta'] = np.ones(C, np.float32), np.zeros(C, np.float32)
        d['mean'], d['invstd'] = np.zeros(C, np.float32), np.ones(C, np.float32)
        return d
    yshape = (N, C, H, W) if variant == 'bcast' else (T, N, C, H, W)
    d['y'] = (rng.standard_normal(yshape) * 1.5 + 0.3).astype(np.float32)
    d['g_s'] = rng.standard_normal((T, N, C, H, W)).astype(np.float32)
    d['gamma'] = rng.uniform(0.8, 1.6, C).astype(np.float32)
    d['beta'] = rng.uniform(-0.1, 0.6, C).astype(np.float32)
    if variant == 'grad_mean':
        d['g_mean'] = rng.standard_normal((N, C, H, W)).astype(np.float32)
    if variant == 'v_init':
        d['v_init'] = rng.uniform(-0.5, 0.9, (N, C, H, W)).astype(np.float32)
    y64 = d['y'].astype(np.float64)
    ax = (0, 2, 3) if variant == 'bcast' else (0, 1, 3, 4)
    d['mean'] = y64.mean(axis=ax).astype(np.float32)
    d['invstd'] = (1.0 / np.sqrt(y64.var(axis=ax) + 1e-3)).astype(np.float32)
    return d


def _oracle(d, T, variant, sg, hard, v_reset, detach):
    """fp64 on the CPU: BatchNorm (batch statistics, or the given ones for 'threshold') + PLIF (decay_input = False) over T steps;
    loss = <spikes, g_s> + <mean_t spikes, g_mean>"""
    from oracle import sj_ref
    surrogate = _oracle_surrogate(sg)
    node = sj_ref.ParametricLIFNode(init_tau=2.0, decay_input=False, v_reset=v_reset if hard else None, surrogate_function=surrogate,
                                    detach_reset=detach, step_mode='m').double()
    y = torch.from_numpy(d['y']).double().requires_grad_(True)
    gamma = torch.from_numpy(d['gamma']).double().requires_grad_(True)
    beta = torch.from_numpy(d['beta']).double().requires_grad_(True)
    ys = y.unsqueeze(0).expand(T, *y.shape) if variant == 'bcast' else y
    flat = ys.flatten(0, 1)
    if variant == 'threshold':          # the given statistics (mean 0, invstd 1, gamma 1, beta 0: z = y exactly)
        c = (1, -1, 1, 1)
        z = (flat - torch.from_numpy(d['mean']).double().view(c)) * torch.from_numpy(d['invstd']).double().view(c) * gamma.view(c) + beta.view(c)
    else:
        z = torch.nn.functional.batch_norm(flat, None, None, gamma, beta, training=True, eps=1e-3)
    z = z.view(ys.shape)
    if 'v_init' in d:
        node.v = torch.from_numpy(d['v_init']).double()
    s = node(z)
    loss = (s * torch.from_numpy(d['g_s']).double()).sum()
    if 'g_mean' in d:
        loss = loss + (s.mean(0) * torch.from_numpy(d['g_mean']).double()).sum()
    loss.backward()
    out = dict(spikes=s.detach().numpy(), gy=y.grad.numpy(), ggamma=gamma.grad.numpy(), gbeta=beta.grad.numpy(), gw=float(node.w.grad))
    if sg == 'patan':
        out['ga'] = float(surrogate.inv_sg.alpha.grad)
    return out


def _device_call(dev, d, T, N, C, HW, variant, sg, hard, v_reset, detach):
    """the fused layer's forward (for the spikes) and eas_bn_lif_bwd_ex / _patan through the C ABI"""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    ptr, stream = _lib.ptr, _lib.stream
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    flags = (FLAG_HARD if hard else 0) | (FLAG_DETACH if detach else 0)
    w = torch.zeros((), device=dev)                               # init_tau = 2: k = sigmoid(0) = 1/2
    bcast = int(variant == 'bcast')
    spikes = torch.empty(T, N, C, HW, device=dev)
    rc = L.eas_bn_lif_fwd(ptr(t['y']), ptr(t['mean']), ptr(t['invstd']), ptr(t['gamma']), ptr(t['beta']), ptr(t.get('v_init')), None, ptr(w), 0.0,
                          1.0, float(v_reset), flags & ~FLAG_DETACH, ptr(spikes), None, T, N, C, HW, bcast, stream())
    assert rc == 0
    SENT = 12345.0
    if variant == 'slices':
        # grad_s = channels 3.. of a [T, N, C + 5, HW] tensor, y / grad_y = channels 2.. of [T, N, C + 4, HW] tensors
        gs_big = torch.randn(T, N, C + 5, HW, device=dev)
        gs_big[:, :, 3:3 + C] = t['g_s'].view(T, N, C, HW)
        y_big = torch.randn(T, N, C + 4, HW, device=dev)
        y_big[:, :, 2:2 + C] = t['y'].view(T, N, C, HW)
        gy_big = torch.full((T, N, C + 4, HW), SENT, device=dev)
        gs_p, gs_ctot, y_p, y_ctot, gy_p = gs_big[0, 0, 3].data_ptr(), C + 5, y_big[0, 0, 2].data_ptr(), C + 4, gy_big[0, 0, 2].data_ptr()
    else:
        gy = torch.full(tuple(t['y'].shape), SENT, device=dev)
        gs_p, gs_ctot, y_p, y_ctot, gy_p = ptr(t['g_s']), 0, ptr(t['y']), 0, ptr(gy)
    ggamma, gbeta, gw = torch.empty(C, device=dev), torch.empty(C, device=dev), torch.empty((), device=dev)
    ws = torch.empty(L.eas_bn_workspace_doubles(C), dtype=torch.float64, device=dev)
    batch_stats = int(variant != 'threshold')
    head = (gs_p, gs_ctot, ptr(t.get('g_mean')), y_p, y_ctot, ptr(t['mean']), ptr(t['invstd']), ptr(t['gamma']), ptr(t['beta']), ptr(t.get('v_init')),
            ptr(w), 0.0, 1.0, float(v_reset), flags)
    tail = (batch_stats, gy_p, ptr(ggamma), ptr(gbeta), ptr(gw), ptr(ws), T, N, C, HW, bcast, stream())
    ga = None
    with ops.kernel_trace() as tr:
        if sg == 'patan':
            alpha = torch.tensor([ALPHA[sg]], device=dev)
            ga = torch.empty(1, device=dev)
            rc = L.eas_bn_lif_bwd_patan(*head, ptr(alpha), ptr(ga), *tail)
        else:
            rc = L.eas_bn_lif_bwd_ex(*head, SG[sg], ALPHA[sg], *tail)
    assert rc == 0
    torch.cuda.synchronize()
    if variant == 'slices':
        rest = torch.cat([gy_big[:, :, :2], gy_big[:, :, 2 + C:]], dim=2)
        assert bool((rest == SENT).all()), 'the backward wrote outside its channel slice of grad_y'
        gy = gy_big[:, :, 2:2 + C].contiguous()
    assert not bool((gy == SENT).any()), 'grad_y was not written everywhere'
    out = dict(spikes=spikes.cpu().numpy(), gy=gy.cpu().numpy(), ggamma=ggamma.cpu().numpy(), gbeta=gbeta.cpu().numpy(), gw=gw.cpu().numpy().copy())
    if ga is not None:
        out['ga'] = ga.cpu().numpy().copy()
    return out, [k for k in tr.kernels if 'bn_lif_bwd' in k]


def _check(dev, monkeypatch, T, N, C, HW, variant, sg, hard, v_reset, detach, one_pass):
    d = _inputs(T, N, C, HW, variant, seed=T * 1000 + C * 10 + HW + len(variant), v0=v_reset if hard else 0.0)
    ref = _oracle(d, T, variant, sg, hard, v_reset, detach)
    monkeypatch.delenv('EAS_BNLIF_BWD', raising=False)
    got, kernels = _device_call(dev, d, T, N, C, HW, variant, sg, hard, v_reset, detach)
    # the form and the instance the table promises
    assert kernels and all(('bn_lif_bwd_small_kernel' in k) == (one_pass and variant != 'bcast') for k in kernels if 'scalars' not in k), kernels
    # (the one-pass kernel reads its optional operands in front of its passes: its fast instance takes every operand form)
    fast = sg == 'atan' and not hard and not detach and T in FAST_T and (variant in PLAIN_VARIANTS or (one_pass and variant != 'bcast'))
    want = 'BnLifBwdPolicy<0, false>' if fast else 'BnLifBwdPolicy<-1, false>'
    assert all(want in k for k in kernels if 'scalars' not in k), (want, kernels)
    # ---- the yardstick: the fp64 oracle
    g_np = d['g_s'].reshape(ref['spikes'].shape).astype(np.float64)
    if 'g_mean' in d:
        g_np = g_np + d['g_mean'].astype(np.float64)[None] / T
    flips = got['spikes'].reshape(ref['spikes'].shape) != ref['spikes']
    if variant == 'threshold':
        assert not flips.any(), 'dyadic inputs: fp32 and fp64 must fire alike, the steps exactly on the threshold included'
        assert (ref['spikes'][0, :, :, 0, 0] == 1).all()          # h = v_th exactly: fires
    assert flips.mean() < 1e-3
    nflip = int(flips.any(axis=0).sum())
    slack = nflip * T * float(np.abs(g_np).max()) * 2.0
    same = ~flips.any(axis=0)
    gy, gy_ref = got['gy'].reshape(ref['gy'].shape), ref['gy']
    if variant != 'bcast':
        same = np.broadcast_to(same, flips.shape)
    np.testing.assert_allclose(gy[same], gy_ref[same], rtol=2e-3, atol=2e-5 + (1e-3 if nflip else 0.0))
    np.testing.assert_allclose(got['ggamma'], ref['ggamma'], rtol=2e-3, atol=2e-4 + slack)
    np.testing.assert_allclose(got['gbeta'], ref['gbeta'], rtol=2e-3, atol=2e-4 + slack)
    np.testing.assert_allclose(float(got['gw']), ref['gw'], rtol=2e-3, atol=1e-4 + slack)
    if sg == 'patan':
        np.testing.assert_allclose(float(got['ga'].reshape(-1)[0]), ref['ga'], rtol=2e-3, atol=1e-4 + slack)
    # ---- extra: the generic instance on the same inputs, bit for bit
    if fast:
        monkeypatch.setenv('EAS_BNLIF_BWD', 'generic')
        gen, gk = _device_call(dev, d, T, N, C, HW, variant, sg, hard, v_reset, detach)
        assert all('BnLifBwdPolicy<-1, false>' in k for k in gk if 'scalars' not in k), gk
        for key in ('gy', 'ggamma', 'gbeta', 'gw'):
            assert got[key].tobytes() == gen[key].tobytes(), f'{key}: the fast instance and the generic instance differ'


# (surrogate, hard reset, v_reset, detached reset): all four surrogates, both resets (hard with and without a reset potential), both
# reset forms.  The first row is the one the table has fast instances for.
NEURONS = [('atan', False, 0.0, False), ('atan', False, 0.0, True), ('atan', True, 0.0, False), ('atan', True, -0.5, True),
           ('sigmoid', False, 0.0, False), ('sigmoid', True, 0.0, True), ('rect', False, 0.0, False), ('rect', True, -0.5, True),
           ('patan', False, 0.0, False), ('patan', True, 0.0, False), ('patan', False, 0.0, True)]
VARIANTS = ('plain', 'grad_mean', 'v_init', 'slices', 'bcast', 'threshold')
# (form, N, C, HW); HW = None: the first one-pass size that takes 512-thread blocks at this T
SHAPES = [('two', 2, 9, 8), ('two', 2, 9, 12), ('one', 2, 64, 8), ('one', 2, 64, None)]


@pytest.mark.parametrize('neuron', NEURONS, ids=lambda n: f'{n[0]}-{"hard" if n[1] else "soft"}{n[2]:g}-{"detached" if n[3] else "attached"}')
@pytest.mark.parametrize('form,N,C,HW', SHAPES)
@pytest.mark.parametrize('T', [1, 3, 4])
def test_bn_lif_bwd_instance_vs_oracle(dev, monkeypatch, T, form, N, C, HW, neuron):
    sg, hard, v_reset, detach = neuron
    hw = _one_pass_512_hw(T) if HW is None else HW
    for variant in VARIANTS:
        _check(dev, monkeypatch, T, N, C, hw, variant, sg, hard, v_reset, detach, form == 'one')


@pytest.mark.parametrize('neuron', [NEURONS[0], NEURONS[5]], ids=['fast', 'generic'])
@pytest.mark.parametrize('form,N,C,HW', SHAPES)
@pytest.mark.parametrize('T', [5, 7])
def test_bn_lif_bwd_fast_instances_of_the_longer_sequences_vs_oracle(dev, monkeypatch, T, form, N, C, HW, neuron):
    """the table's fast instances for T = 5 and T = 7 (bench configurations 3 and 5), next to a generic row of the same T"""
    sg, hard, v_reset, detach = neuron
    hw = _one_pass_512_hw(T) if HW is None else HW
    for variant in VARIANTS:
        _check(dev, monkeypatch, T, N, C, hw, variant, sg, hard, v_reset, detach, form == 'one')
