"""Depthwise 3x3 convolution kernels (eas_dwconv_*, csrc/dwconv.hip) on the MI355X: exactness on spikes for both input forms with the
statistics epilogue, real values against torch's fp64 CPU convolution through ``ops.conv2d`` and autograd, reproducibility, a converted
DWConv block against the library route (``ctx.dwconv`` off), HIP-graph capture, and a whole depthwise=True model on the native route.

Shapes are the smallest at which the decomposition can go wrong: one pixel, odd sizes at both strides, a partial last channel group
(fp32 form), several channel groups, several images per tile, rows wide enough for more than one row band."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (NI, C, H, W, stride)
CASES = [(1, 8, 1, 1, 1), (2, 8, 5, 7, 1), (2, 8, 5, 7, 2), (3, 24, 8, 10, 1), (2, 16, 7, 9, 2), (1, 40, 16, 20, 2), (2, 64, 8, 10, 1),
         (1, 8, 2, 320, 1), (1, 8, 6, 130, 2)]
FP32_ONLY_CASES = [(2, 5, 5, 7, 1), (2, 5, 6, 9, 2), (1, 12, 8, 10, 1), (2, 12, 7, 9, 2)]       # C = 5 and C = 12: a partial channel group
BIG_CASES = [(8, 8, 64, 80, 1), (4, 16, 33, 47, 2)]          # a tap sum of >= 40 000 terms; odd sizes at stride 2 with several bands
DW_CALLS = ('eas_dwconv_fwd', 'eas_dwconv_fwd_planes', 'eas_dwconv_dgrad', 'eas_dwconv_wgrad', 'eas_dwconv_wgrad_planes')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


def _id(case):
    return 'x'.join(str(v) for v in case)


def _spike_case(case):
    """x in {0,1,2}, w in multiples of 1/8 in [-1,1]: every partial sum is exact in fp32 (and its square sum in fp64), so the fp64
    reference is THE result of any correct kernel, whatever its order of additions (confirmed on the CPU in tests/test_cpu_dwconv.py)"""
    NI, C, H, W, s = case
    g = torch.Generator().manual_seed(NI * 1000 + C * 100 + H * 10 + W + s)
    x = torch.randint(0, 3, (NI, C, H, W), generator=g).float()
    w = torch.randint(-8, 9, (C, 1, 3, 3), generator=g).float() / 8
    y64 = F.conv2d(x.double(), w.double(), None, s, 1, 1, C)
    return x, w, y64


def _as_planes(x):
    """[NI,C,H,W] fp32 spikes -> planes [NI,C/8,H*W,8] bf16: ``ops.to_planes`` where it takes the map (H*W in whole fours), else the same
    layout written with torch (the depthwise kernels read planes of any H*W)"""
    from eas_snn_amd import ops
    NI, C, H, W = x.shape
    if (H * W) % 4 == 0:
        return ops.to_planes(x)
    return x.view(NI, C // 8, 8, H * W).permute(0, 1, 3, 2).contiguous().to(torch.bfloat16)


def _run_fwd(L, form, xin, w, case, with_stats, dev, nb_delta=0):
    from eas_snn_amd.ops import ptr, stream
    NI, C, H, W, s = case
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    y = torch.full((NI, C, Ho, Wo), float('nan'), device=dev)
    nb = L.eas_dwconv_fwd_stats_blocks(NI, C, H, W, s, form) if with_stats else 0
    stats = torch.full((C, max(nb + nb_delta, 1), 2), float('nan'), dtype=torch.float64, device=dev) if with_stats else None
    fn = L.eas_dwconv_fwd_planes if form == 2 else L.eas_dwconv_fwd
    rc = fn(ptr(xin), ptr(w), None, ptr(y), NI, C, H, W, s, ptr(stats), nb + nb_delta if with_stats else 0, stream())
    return rc, y, stats, nb


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_spikes_are_exact_in_both_forms_with_statistics(dev, case):
    import eas_snn_amd
    from eas_snn_amd import ops
    L = eas_snn_amd.hip_library()
    NI, C, H, W, s = case
    x, w, y64 = _spike_case(case)
    ref = y64.float()
    xd, wd = x.to(dev), w.to(dev)
    sp = _as_planes(xd)
    want_s, want_q = y64.sum((0, 2, 3)), (y64 * y64).sum((0, 2, 3))
    for form, xin in ((2, sp), (1, xd)):
        assert L.eas_dwconv_supported(NI, C, H, W, s, form) == 1
        rc, y, stats, nb = _run_fwd(L, form, xin, wd, case, True, dev)
        assert rc == 0 and nb > 0
        assert torch.equal(y.cpu(), ref), f'form {form}: max abs diff {float((y.cpu() - ref).abs().max())}'
        st = stats.cpu().sum(1)
        assert torch.equal(st[:, 0], want_s) and torch.equal(st[:, 1], want_q), f'form {form}'
        rc, y, _, _ = _run_fwd(L, form, xin, wd, case, False, dev)
        assert rc == 0 and torch.equal(y.cpu(), ref)
        rc, y, stats, _ = _run_fwd(L, form, xin, wd, case, True, dev, nb_delta=1)          # a wrong nb is refused before anything is launched
        assert rc != 0 and bool(torch.isnan(y).all()) and bool(torch.isnan(stats).all())
    # the operator route on a ghost: planes form, statistics handed over through the slot
    conv = nn.Conv2d(C, C, 3, s, 1, groups=C, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(wd)
        gx = ops.ghost(xd.shape, dev, sp)
        with ops.kernel_trace() as tr, ops.conv_stats_scope(True):
            y = ops.conv2d(gx, conv)
        slot = ops.ctx.conv_stats_slot
        ops.clear_conv_stats()
    assert [c[0] for c in tr.calls] == ['eas_dwconv_fwd_planes']
    assert torch.equal(y.cpu(), ref)
    assert slot is not None and slot[0] is y and torch.equal(slot[2].view(C, slot[1], 2).sum(1)[:, 0].cpu(), want_s)


@pytest.mark.parametrize('case', FP32_ONLY_CASES, ids=_id)
def test_fp32_form_takes_any_channel_count(dev, case):
    import eas_snn_amd
    L = eas_snn_amd.hip_library()
    NI, C, H, W, s = case
    x, w, y64 = _spike_case(case)
    assert L.eas_dwconv_supported(NI, C, H, W, s, 1) == 1 and L.eas_dwconv_supported(NI, C, H, W, s, 2) == 0
    rc, y, _, _ = _run_fwd(L, 1, x.to(dev), w.to(dev), case, False, dev)
    assert rc == 0 and torch.equal(y.cpu(), y64.float())


def _real_case(case, bias):
    NI, C, H, W, s = case
    g = torch.Generator().manual_seed(7 + NI + C + H + W + s)
    x = torch.randn(NI, C, H, W, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3
    b = torch.randn(C, generator=g) if bias else None
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    gy = torch.randn(NI, C, Ho, Wo, generator=g)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if bias else None
    y64 = F.conv2d(x64, w64, b64, s, 1, 1, C)
    y64.backward(gy.double())
    return x, w, b, gy, y64.detach(), x64.grad, w64.grad, (b64.grad if bias else None)


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


@pytest.mark.parametrize('case', CASES + BIG_CASES, ids=_id)
def test_real_values_against_fp64_through_conv2d_and_autograd(dev, case):
    """max abs error < 1e-5 of the reference's max magnitude for y, grad_x and grad_w: the project's tolerance for its dense convolutions
    (test_conv_mfma_forward_dgrad_wgrad_vs_fp64)"""
    from eas_snn_amd import ops
    NI, C, H, W, s = case
    bias = case == (2, 16, 7, 9, 2)
    x, w, b, gy, y64, gx64, gw64, gb64 = _real_case(case, bias)
    conv = nn.Conv2d(C, C, 3, s, 1, groups=C, bias=bias).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w.to(dev))
        if bias:
            conv.bias.copy_(b.to(dev))
    xd = x.to(dev).requires_grad_(True)
    with ops.kernel_trace() as tr:
        y = ops.conv2d(xd, conv)
        y.backward(gy.to(dev))
    names = [c[0] for c in tr.calls]
    assert 'eas_dwconv_fwd' in names and 'eas_dwconv_dgrad' in names and 'eas_dwconv_wgrad' in names, names
    errs = dict(y=_rel(y.detach(), y64), gx=_rel(xd.grad, gx64), gw=_rel(conv.weight.grad, gw64))
    if bias:
        errs['gb'] = _rel(conv.bias.grad, gb64)
    print(f'{_id(case)}: {errs}')
    assert all(e < 1e-5 for e in errs.values()), errs


def test_switch_off_is_the_library_route(dev):
    from eas_snn_amd import ops
    case = (2, 16, 7, 9, 2)
    NI, C, H, W, s = case
    x, w, b, gy, y64, gx64, gw64, _ = _real_case(case, False)
    conv = nn.Conv2d(C, C, 3, s, 1, groups=C, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w.to(dev))
    xd = x.to(dev).requires_grad_(True)
    prev, ops.ctx.dwconv = ops.ctx.dwconv, False
    try:
        with ops.kernel_trace() as tr:
            y = ops.conv2d(xd, conv)
            y.backward(gy.to(dev))
    finally:
        ops.ctx.dwconv = prev
    assert not any(c[0] in DW_CALLS for c in tr.calls), tr.calls
    assert not any('dwconv' in k for k in tr.kernels), tr.kernels
    assert _rel(y.detach(), y64) < 1e-5 and _rel(xd.grad, gx64) < 1e-5 and _rel(conv.weight.grad, gw64) < 1e-5


def test_backward_is_bit_reproducible(dev):
    from eas_snn_amd import ops
    case = (3, 24, 8, 10, 1)
    NI, C, H, W, s = case
    x, w, b, gy, *_ = _real_case(case, False)
    conv = nn.Conv2d(C, C, 3, s, 1, groups=C, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w.to(dev))
    runs = []
    for _ in range(2):
        conv.weight.grad = None
        xd = x.to(dev).requires_grad_(True)
        ops.conv2d(xd, conv).backward(gy.to(dev))
        runs.append((xd.grad.clone(), conv.weight.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    sp = _as_planes((x.to(dev) > 0).float())                        # the planes form of the weight gradient as well
    xs = (x.to(dev) > 0).float()
    gws = []
    for _ in range(2):
        gws.append(ops.dwconv_wgrad(xs, gy.to(dev), s, sp).clone())
    assert torch.equal(gws[0], gws[1])
    assert torch.equal(gws[0], ops.dwconv_wgrad(xs, gy.to(dev), s, None))        # same image in LDS, same order: planes == fp32 bit for bit


class _Block(nn.Module):
    """a spiking BaseConv in front of a DWConv: the input of ``dconv`` arrives as spike planes"""

    def __init__(self, stride):
        super().__init__()
        from yolox.models.network_blocks import BaseConv, DWConv
        self.pre = BaseConv(16, 16, 3, 1)
        self.dw = DWConv(16, 32, 3, stride)

    def forward(self, x):
        return self.dw(self.pre(x))


def _make_block(stride, dev):
    from spikingjelly.activation_based import surrogate
    from yolox.models.network_blocks import enable_spike_planes
    from yolox.utils.utils_snn import convert_to_spiking
    torch.manual_seed(11 + stride)
    net = convert_to_spiking(_Block(stride), surrogate.ATan(2.0))
    enable_spike_planes(net)
    with torch.no_grad():
        dconv = net.dw.dconv.conv[0]
        assert isinstance(dconv, nn.Conv2d) and dconv.groups == 16
        dconv.weight.copy_(torch.randint(-8, 9, dconv.weight.shape).float() / 8)
        net.pre.conv[0].weight.mul_(3.0)                   # keep the block firing
        net.dw.pconv.conv[0].weight.mul_(3.0)
    return net.to(dev)


def _run_block(net, state, x, g_out, train, dev):
    from eas_snn_amd import ops
    from spikingjelly.activation_based import functional
    net.load_state_dict(state)
    net.zero_grad(set_to_none=True)
    net.train(train)
    xs = ops.mark_small_int(x.clone())
    with ops.kernel_trace() as tr:
        if train:
            with ops.packed_weights(net):
                out = ops.dense(net(xs))
            (out * g_out).sum().backward()
        else:
            with torch.no_grad(), ops.packed_weights(net):
                out = ops.dense(net(xs))
    functional.reset_net(net)
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    bufs = {n: b.clone() for n, b in net.named_buffers()}
    return out.detach().clone(), grads, bufs, [c[0] for c in tr.calls]


@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('stride', [1, 2])
def test_spiking_dwconv_block_against_the_library_route(dev, stride, train):
    """dconv's y is exact on both routes (spikes x multiples of 1/8), so are the statistics: the two routes must give the same spikes and
    running statistics bit for bit, and parameter gradients that differ by summation order only"""
    from eas_snn_amd import ops
    net = _make_block(stride, dev)
    state = copy.deepcopy(net.state_dict())
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(3, 2, 16, 16, 20, generator=g) < 0.4).float().to(dev)
    Ho, Wo = (16 - 1) // stride + 1, (20 - 1) // stride + 1
    g_out = torch.randn(3, 2, 32, Ho, Wo, generator=g).to(dev)
    on = _run_block(net, state, x, g_out, train, dev)
    prev, ops.ctx.dwconv = ops.ctx.dwconv, False
    try:
        off = _run_block(net, state, x, g_out, train, dev)
    finally:
        ops.ctx.dwconv = prev
    assert 0.0 < float(on[0].mean()) < 1.0, 'the block must fire for this test to mean something'
    assert torch.equal(on[0], off[0])
    for n in on[2]:
        assert torch.equal(on[2][n], off[2][n]), n
    if train:
        assert set(on[1]) == set(off[1]) and 'dw.dconv.conv.0.weight' in on[1]
        for n in on[1]:
            assert _rel(on[1][n], off[1][n].double().cpu()) < 1e-5, n
    # switch on: dconv read the producer's planes -- nothing was unpacked in front of it, and its BatchNorm took the epilogue's sums
    calls = on[3]
    assert 'eas_dwconv_fwd_planes' in calls and 'eas_dwconv_fwd' not in calls, calls
    assert 'eas_spike_planes_to_f32' not in calls[:calls.index('eas_dwconv_fwd_planes')], calls
    assert not any(c in DW_CALLS for c in off[3]) and 'eas_spike_planes_to_f32' in off[3][:-1], off[3]
    if train:
        assert 'eas_dwconv_dgrad' in calls and 'eas_dwconv_wgrad_planes' in calls
        assert calls.count('eas_bn_stats_partial') < off[3].count('eas_bn_stats_partial'), (calls, off[3])


def test_forward_and_backward_capture_into_a_graph(dev):
    """forward (statistics epilogue -> BN+LIF) and backward of a converted depthwise BaseConv recorded on one stream, replayed twice"""
    from eas_snn_amd import ops
    from spikingjelly.activation_based import functional, surrogate
    from yolox.models.network_blocks import BaseConv
    from yolox.utils.utils_snn import convert_to_spiking
    NI, C, H, W, s = 2, 16, 7, 9, 2
    torch.manual_seed(5)
    blk = convert_to_spiking(BaseConv(C, C, 3, s, groups=C), surrogate.ATan(2.0)).to(dev).train()
    with torch.no_grad():
        blk.conv[0].weight.mul_(3.0)
    g = torch.Generator().manual_seed(9)
    x = ops.mark_small_int((torch.rand(2, 1, C, H, W, generator=g) < 0.5).float().to(dev)).requires_grad_(True)
    g_out = torch.randn(2, 1, C, 4, 5, generator=g).to(dev)

    def step():
        out = blk(x)
        out.backward(g_out)
        functional.reset_net(blk)
        return out

    with ops.kernel_trace() as tr:
        ref = step().detach().clone()
    fwd = [c for c in tr.calls if c[0] == 'eas_dwconv_fwd']
    assert len(fwd) == 1 and fwd[0][1][9] is not None, 'the convolution must hand its statistics to the BN+LIF kernel'
    assert not any(c[0] == 'eas_bn_stats_partial' for c in tr.calls)
    assert 0.0 < float(ref.mean()) < 1.0
    ref_gx, ref_gw = x.grad.clone(), blk.conv[0].weight.grad.clone()
    x.grad = None
    blk.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.detach(), ref)
        assert torch.equal(x.grad, ref_gx) and torch.equal(blk.conv[0].weight.grad, ref_gw)


def _depthwise_model(dev):
    """SpikingYOLOPAFPN(depth 0.33, width 0.25, depthwise=True) + a depthwise=True head, assembled as the experiment assembles its models"""
    from oracle import fill
    from yolox.exp import get_exp
    from yolox.models import SpikingYOLOPAFPN, SpikingYOLOX, YOLOXHead
    from yolox.models.network_blocks import enable_spike_planes
    exp = get_exp(None, 'e-yolox-s')
    exp.merge(['T', '2', 'embedding', 'arsnn', 'num_classes', '2', 'spike_attach', 'True', 'thresh', '1', 'readout', 'sum', 'embedding_depth', '2',
               'embedding_ksize', '5', 'write_zero', 'True', 'spike_fn', 'atan', 'use_spike', 'True', 'input_size', '(64,64)', 'test_size', '(64,64)'])
    chans = [256, 512, 1024]
    backbone = SpikingYOLOPAFPN(0.33, 0.25, in_channels=chans, in_dim=exp.in_dim, act=exp.act, spike_fn=exp.get_act_func(), depthwise=True)
    head = YOLOXHead(exp.num_classes, 0.25, in_channels=chans, act=exp.act, depthwise=True)
    model = SpikingYOLOX(backbone, head, exp._build_embedding(), T=exp.T)
    enable_spike_planes(model)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eps, m.momentum = 1e-3, 0.03
    model.head.initialize_biases(1e-2)
    fill.procedural_fill_(model, 2.0, ann_regex=fill.ANN_KEYS['True'])
    return model.to(dev).train()


def test_depthwise_model_trains_on_the_native_route(dev):
    """SpikingYOLOPAFPN(depthwise=True) + a depthwise=True head: every grouped convolution of a training step runs on eas_dwconv_*.
    (No end-to-end closeness between the two routes is asserted: a deep spiking model diverges from a single near-threshold flip; parity
    is asserted per layer above.)"""
    from eas_snn_amd import data, ops
    from oracle import fill
    from spikingjelly.activation_based import functional
    model = _depthwise_model(dev)
    grouped = [m for m in model.modules() if isinstance(m, nn.Conv2d) and m.groups > 1]
    assert len(grouped) >= 20 and all(ops.dwconv_form_ok(m) for m in grouped)
    x = torch.from_numpy(fill.poisson_events((2, 1, 4, 2, 64, 64), 0.5, seed=3)).to(dev)
    tg = data.synth_targets(2, (64, 64), dev)
    # a third box of canvas size: without it no anchor of the stride-32 level (2x2 cells) is assigned a target and the class branch of that
    # level gets an exactly zero gradient on ANY route (the loss's doing, not a convolution's)
    tg[:, 2] = torch.tensor([0.0, 32.0, 32.0, 56.0, 56.0], device=dev)
    with ops.kernel_trace() as tr:
        out = model(x, tg)
        out['total_loss'].backward()
    functional.reset_net(model)
    assert bool(torch.isfinite(out['total_loss']))
    nfwd = sum(1 for c in tr.calls if c[0] in ('eas_dwconv_fwd', 'eas_dwconv_fwd_planes'))
    assert nfwd == len(grouped), (nfwd, len(grouped))
    assert any(c[0] == 'eas_dwconv_fwd_planes' for c in tr.calls) and any(c[0] == 'eas_dwconv_fwd' for c in tr.calls)
    for m in grouped:
        assert m.weight.grad is not None and bool(torch.isfinite(m.weight.grad).all()) and float(m.weight.grad.abs().max()) > 0.0
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
