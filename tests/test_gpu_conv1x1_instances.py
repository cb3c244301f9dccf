"""conv1x1_mfma.hip: every kernel instance the default library can launch, at the smallest shape that reaches it, against fp64.

The launch rules (conv1x1_dispatch_t, eas_conv1x1_lif_dispatch, eas_conv1x1_group, w1_plan) pick an instance from NI, Cin, Cout and HW.  Every
case here (1) runs under ``ops.kernel_trace()`` and asserts the traced symbol, cut down as ``test_gpu_bench_shapes._short`` does, carries exactly
the template arguments the case promises -- a shape that lands on another instance fails; (2) writes into NaN-filled outputs and finds no NaN
left (a channel slice of a wider tensor: the rest keeps its sentinel); (3) compares with ``torch.nn.functional.conv2d`` /
``torch.nn.grad.conv2d_input`` / ``conv2d_weight`` in double on the device at the project's bar, max |difference| / max |reference| < 1e-5; (4) makes
the same call twice and requires the same bits.  The first call goes through the operator (``ops.conv_fwd_packed``, ``ops.conv_wgrad``), whose
output is allocated inside; the second is the same call on the C ABI into the NaN-filled output.

Instances and the cases that launch them (``<..>`` = the template arguments asserted):

plain forward / input gradient, LM = 0 -- test_plain_forward[instance-operand], PLAIN_SHAPES; XT = 3 (fp32, three terms), XT = 1 (fp32 small
integers), PL (spike planes from ``ops.to_planes``, also bit-identical to XT = 1); the fp32 case runs the instance a second time as an input
gradient (weights packed transposed) against ``conv2d_input``:
  conv1x1_mfma_kernel<XT, WM, WN, false, PL, 0>        (WM, WN) in (4,2) (2,2) (1,2) (4,1) (2,1) (1,1)       18 instances
  conv1x1_mfma_sharedA_kernel<XT, WM, WN, PL, 0>       (WM, WN) in (4,2) (4,1) (2,1)                          9 instances
  conv1x1_mfma_kernel<XT, WM, 1, true, false, 0>       ragged Cin, WM in 4, 2, 1, XT in 3, 1                   6 instances: test_ragged_input_channels
  the channel loop's 0 / 1 / 2 trips and its tail step on <.., 1, 1, ..>: test_channel_loop_edges (Cin 8, 16, 24, 40, 48)
  bias, statistics epilogue and SiLU epilogue are run-time branches of the same instances: test_epilogues, once per (WM, WN) of both forms
  left out: sharedA<.., 2, 2, ..>.  launch_c1_shared names it, but the default rule keeps sn = 2 only while sm stays 4; only the development
  override EAS_C1_SHARED_SHAPE reaches it and the default library compiles that out.  (A later simplification may drop the instance.)

fused eval step, LM = 1 -- tests/test_gpu_kernels.py::test_fused_eval_step_is_bit_identical_to_conv_then_bn_lif, FUSED_EVAL_1X1_INSTANCES there
(bit identity with the unfused composition, which the plain cases here tie to fp64):
  conv1x1_mfma_kernel<1, 1, 3|5, false, true, 1>, conv1x1_mfma_kernel<1, 2, 3|5, false, true, 1>, conv1x1_mfma_sharedA_kernel<1, 2, 3|5, true, 1>

BatchNorm + activation epilogue, LM = 3 -- tests/test_gpu_kernels.py::test_fused_real_valued_eval_block_is_bit_identical_to_conv_then_bn_silu,
FUSED_ANN_1X1_INSTANCES there:
  conv1x1_mfma_kernel<3, 1, 1, false, false, 3>, <3, 1, 2, ..>, conv1x1_mfma_sharedA_kernel<3, 2, 1, false, 3>, <3, 4, 1, ..>, <3, 4, 2, ..>
  left out: the direct (2,1) (4,1) (2,2) (4,2) tiles with LM = 3 (the same tile body as LM = 0, whose every tile is covered above, and the same
  epilogue as the rows listed; the bench-shape replay reaches those a bench step launches) and the grouped LM = 3 kernels
  (test_grouped_bn_silu_forward_backward_vs_fp64).

grouped launches, eas_conv_fwd_group with ksize 1 -- conv1x1_group_kernel<3, WM, WN, RAGK, 0, C1GeomCore>.  From the trace of
test_grouped_convolution_equals_the_single_launches at its batches 3 and 64: forward <3, 1, 1, false, ..> and <3, 4, 1, false, ..>, input
gradient <3, 1, 1, false, ..> and <3, 4, 2, false, ..>; test_grouped_prediction_convolutions_bias_ragged_channels_and_accumulation (batch 16) adds
<3, 1, 1, true, ..>.  Not run there: <3, 2, 1, false, ..> and the ragged <3, 4, 1, true, ..>: test_grouped_launch[tile21] / [ragged41] here;
[mixed] is a group of MT = 1 and MT = 4 problems (the wave tile follows the narrowest: <3, 1, 1, false, ..>).

weight gradient (single launch) -- test_wgrad_instances: conv1x1_wgrad_lds_kernel<XT, WVM, WVN, NT, KS, XPL>, block shape (1,4,1) (2,2,2) (4,1,4)
by Cout 24 / 40 / 72, KS 1 / 2 by HW 48 / 64, operand <3, .., false>, <1, .., false>, <1, .., true>: all 18.  test_wgrad_two_input_channel_blocks
(Cin = 136), test_wgrad_short_last_slice_across_images (NI = 3, a slice count that does not divide the chunk count) and test_wgrad_refusals run on
the same instances.  The grouped weight-gradient kernel has test_grouped_weight_gradient_slabs_vs_fp64."""

import functools
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

OPERANDS = ('f32', 'int', 'planes')          # fp32 three terms (XT = 3), fp32 small integers (XT = 1), spike planes (XT = 1, PL)
SENT = 12345.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    yield torch.device('cuda:0')
    _case.cache_clear()


def _short(sym):
    """'void (anonymous namespace)::conv1x1_mfma_kernel<3, 4, 2, ...>(float const*, ...)' -> 'conv1x1_mfma_kernel<3, 4, 2, ...>'"""
    s = re.sub(r'^void\s+', '', sym).replace('(anonymous namespace)::', '')
    depth, out = 0, []
    for ch in s:                                    # cut the argument list: the first '(' outside template brackets
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            break
        out.append(ch)
    return ''.join(out).strip()


def _traced(tr, family='conv1x1_'):
    return sorted({_short(k) for k in tr.kernels if family in k})


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _conv64(x, w, b=None):
    """fp64 1x1 convolution on the device (ATen: no library of ours involved), on the host if the device refuses"""
    try:
        return torch.nn.functional.conv2d(x.double(), w.double(), None if b is None else b.double())
    except RuntimeError:
        return torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), None if b is None else b.double().cpu()).to(x.device)


@functools.lru_cache(maxsize=None)
def _case(shape, ints):
    """inputs of one shape and their fp64 convolution, made once and shared by the cases that read them (nothing writes to them)"""
    NI, Cin, Cout, H, W = shape
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(NI * 1009 + Cin * 31 + Cout * 7 + H * W + int(ints))
    x = torch.randint(0, 4, (NI, Cin, H, W), generator=g).float() if ints else torch.randn(NI, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    b = torch.randn(Cout, generator=g)
    x, w, b = x.to(dev), w.to(dev), b.to(dev)
    return x, w, b, _conv64(x, w)


def _symbol(form, wm, wn, op, ragk=False, lm=0):
    xt, pl = (3 if op == 'f32' else 1), ('true' if op == 'planes' else 'false')
    if form == 'shared':
        return f'conv1x1_mfma_sharedA_kernel<{xt}, {wm}, {wn}, {pl}, {lm}>'
    return f'conv1x1_mfma_kernel<{xt}, {wm}, {wn}, {"true" if ragk else "false"}, {pl}, {lm}>'


def _abi_forward(xin, pk, bias, y, shape, op, act=0, stats=None, nb=0):
    """the C-ABI call ``ops.conv_fwd_packed`` makes for this operand form, writing into the caller's ``y``"""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    NI, Cin, Cout, H, W = shape
    p, xt = ops.ptr, (3 if op == 'f32' else 1)
    if op == 'planes':
        assert not act
        rc = L.eas_conv_fwd_planes(p(xin), p(pk), p(bias), p(y), NI, Cin, Cout, H, W, 1, 1, p(stats), nb, ops.stream())
    elif act:
        rc = L.eas_conv_fwd_act(p(xin), p(pk), p(bias), p(y), NI, Cin, Cout, H, W, 1, 1, xt, act, None, ops.stream())
    elif stats is not None:
        rc = L.eas_conv_fwd_stats(p(xin), p(pk), p(y), NI, Cin, Cout, H, W, 1, 1, xt, None, p(stats), nb, ops.stream())
    else:
        rc = L.eas_conv_fwd(p(xin), p(pk), p(bias), p(y), NI, Cin, Cout, H, W, 1, 1, xt, None, ops.stream())
    assert rc == 0, rc


def _forward(shape, op, want, x, w, bias=None):
    """y of the traced operator call; the instance, 'written everywhere' and 'same bits twice' are asserted here"""
    from eas_snn_amd import ops
    NI, Cin, Cout, H, W = shape
    pk = ops.conv_pack_weights(w, 0)
    sp = ops.to_planes(x) if op == 'planes' else None
    with ops.kernel_trace() as tr:
        y = ops.conv_fwd_packed(x, pk, bias, Cout, 1, 1, 3 if op == 'f32' else 1, sp)
    assert _traced(tr) == [want], (shape, op, _traced(tr))
    y2 = torch.full_like(y, float('nan'))
    _abi_forward(sp if op == 'planes' else x, pk, bias, y2, shape, op)
    assert not torch.isnan(y2).any(), 'y has unwritten elements'
    assert torch.equal(y, y2), 'two identical calls differ'
    return y


# ------------------------------------------------------------------------------------------------ 1. plain forward, LM = 0
# (form, WM, WN) -> (NI, Cin, Cout, H, W): the cheapest shapes the rule of conv1x1_dispatch_t (512 blocks direct, 384 shared, shared from
# Cin >= 256 and MT >= 4) sends to each tile.  Cin = 8: one k-step whose upper half reads the zero page; Cin = 264: 17 k-steps, the register
# pipeline ends on its tail step and the last step is half empty.  Cout 24 / 72 / 136: a ragged last 32-channel tile (136 in the shared form:
# a clamped fragment row).  Every HW but 7 x 160 (35 whole tiles) leaves a ragged last pixel tile, odd widths (121, 139, 199) among them; HW
# stays a multiple of 4 because spike planes exist only for such maps (eas_spike_planes_from_f32); test_ragged_input_channels has an odd HW.
PLAIN_SHAPES = {
    ('direct', 1, 1): (1, 8, 24, 4, 5), ('direct', 1, 2): (16, 8, 24, 68, 121), ('direct', 2, 1): (64, 8, 1024, 9, 4),
    ('direct', 2, 2): (64, 8, 72, 7, 160), ('direct', 4, 1): (32, 8, 136, 8, 139), ('direct', 4, 2): (64, 8, 136, 8, 139),
    ('shared', 2, 1): (1, 264, 136, 4, 5), ('shared', 4, 1): (64, 264, 1024, 6, 12), ('shared', 4, 2): (16, 264, 1024, 4, 199)}
INSTANCES = list(PLAIN_SHAPES)
_inst_id = lambda i: f'{i[0]}{i[1]}{i[2]}'


@pytest.mark.parametrize('op', OPERANDS)
@pytest.mark.parametrize('inst', INSTANCES, ids=_inst_id)
def test_plain_forward(dev, inst, op):
    from eas_snn_amd import ops
    shape = PLAIN_SHAPES[inst]
    x, w, _, y64 = _case(shape, op != 'f32')
    y = _forward(shape, op, _symbol(*inst, op), x, w)
    err = _rel(y, y64)
    assert err < 1e-5, f'{err:.2e}'
    if op == 'planes':          # the same products in the same order as the one-term fp32 form
        assert torch.equal(y, ops.conv_fwd_packed(x, ops.conv_pack_weights(w, 0), None, shape[2], 1, 1, 1))
    if op == 'f32':             # the same instance as an input gradient: grad_y in, the weight [Cin, Cout] of the Cout -> Cin convolution packed transposed
        gy, v = x, w.reshape(shape[2], shape[1]).t().contiguous().reshape(shape[1], shape[2], 1, 1)
        with ops.kernel_trace() as tr:
            gx = ops.conv_fwd_packed(gy, ops.conv_pack_weights(v, 1), None, shape[2], 1, 1, 3)
        assert _traced(tr) == [_symbol(*inst, op)]
        ref = torch.nn.grad.conv2d_input((shape[0], shape[2], shape[3], shape[4]), v.double(), gy.double())
        err = _rel(gx, ref)
        assert err < 1e-5, f'input gradient {err:.2e}'
    assert not ops.tag_violation(dev)


@pytest.mark.parametrize('op', OPERANDS)
@pytest.mark.parametrize('Cin', [8, 16, 24, 40, 48])
def test_channel_loop_edges(dev, Cin, op):
    """1, 1, 2, 3 and 3 k-steps, with and without a half-empty last step: the channel loop's 0, 1 and 2 trips and its tail step"""
    shape = (1, Cin, 24, 4, 5)
    x, w, _, y64 = _case(shape, op != 'f32')
    y = _forward(shape, op, _symbol('direct', 1, 1, op), x, w)
    err = _rel(y, y64)
    assert err < 1e-5, f'{err:.2e}'


@pytest.mark.parametrize('xt', [3, 1])
@pytest.mark.parametrize('Cout,wm', [(32, 1), (64, 2), (136, 4)])
@pytest.mark.parametrize('Cin', [1, 4, 13])
def test_ragged_input_channels(dev, Cin, Cout, wm, xt):
    """RAGK: the input gradient of the 1 / 4 / num_classes-channel prediction convolutions (their 'input' is grad_y with Cin % 8 != 0
    channels), through eas_conv_fwd with the weight packed transposed.  3 x 75 pixels: three pixel blocks, the last with idle waves."""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    NI, H, W = 3, 5, 15
    g = torch.Generator().manual_seed(Cin * 100 + Cout + xt)
    gy = (torch.randint(-2, 3, (NI, Cin, H, W), generator=g).float() if xt == 1 else torch.randn(NI, Cin, H, W, generator=g)).to(dev)
    v = (torch.randn(Cin, Cout, 1, 1, generator=g) / Cin ** 0.5).to(dev)          # the weight of the Cout -> Cin prediction convolution
    pk = ops.conv_pack_weights(v, 1)
    outs = []
    for _ in range(2):
        gx = torch.full((NI, Cout, H, W), float('nan'), device=dev)
        with ops.kernel_trace() as tr:
            rc = L.eas_conv_fwd(ops.ptr(gy), ops.ptr(pk), None, ops.ptr(gx), NI, Cin, Cout, H, W, 1, 1, xt, None, ops.stream())
        assert rc == 0
        assert _traced(tr) == [f'conv1x1_mfma_kernel<{xt}, {wm}, 1, true, false, 0>'], _traced(tr)
        assert not torch.isnan(gx).any(), 'grad_x has unwritten elements'
        outs.append(gx)
    assert torch.equal(*outs)
    ref = torch.nn.grad.conv2d_input((NI, Cout, H, W), v.double(), gy.double())
    err = _rel(outs[0], ref)
    assert err < 1e-5, f'{err:.2e}'


@pytest.mark.parametrize('inst', INSTANCES, ids=_inst_id)
def test_epilogues(dev, inst):
    """bias, BatchNorm statistics and SiLU in the epilogue of every tile of both forms (run-time branches of the plain instances)"""
    import torch.nn as nn
    from eas_snn_amd import ops
    shape = PLAIN_SHAPES[inst]
    NI, Cin, Cout, H, W = shape
    x, w, b, y64 = _case(shape, False)
    want = _symbol(*inst, 'f32')
    plain = _forward(shape, 'f32', want, x, w)
    pk = ops.conv_pack_weights(w, 0)
    # ---- bias
    yb = _forward(shape, 'f32', want, x, w, bias=b)
    ref_b = y64 + b.double().view(1, -1, 1, 1)
    err = _rel(yb, ref_b)
    assert err < 1e-5, f'bias {err:.2e}'
    # ---- statistics: y as the plain call, partial sums = the fp64 sums of that y (the bars of test_conv_epilogue_statistics)
    with ops.kernel_trace() as tr, ops.conv_stats_scope(True):
        ys = ops.conv_fwd_packed(x, pk, None, Cout, 1, 1, 3)
    slot = ops._CONV_STATS_SLOT
    ops.clear_conv_stats()
    assert _traced(tr) == [want], _traced(tr)
    assert slot is not None and slot[0] is ys, 'the convolution left no tile sums'
    nb = slot[1]
    assert torch.equal(ys, plain)
    y2 = torch.full_like(ys, float('nan'))
    st2 = torch.full((Cout * nb * 2,), float('nan'), dtype=torch.float64, device=dev)
    _abi_forward(x, pk, None, y2, shape, 'f32', stats=st2, nb=nb)
    assert torch.equal(y2, plain) and torch.isfinite(st2).all(), 'statistics epilogue: unwritten outputs or partial sums'
    assert torch.equal(st2, slot[2]), 'two identical calls differ'
    got = st2.view(Cout, nb, 2).sum(1)
    p64 = plain.double()
    ssum, ssq = p64.sum((0, 2, 3)), (p64 * p64).sum((0, 2, 3))
    assert float(((got[:, 0] - ssum).abs() / (p64.abs().sum((0, 2, 3)) + 1e-30)).max()) < 3e-7
    assert float(((got[:, 1] - ssq).abs() / (ssq + 1e-30)).max()) < 3e-7
    # ---- SiLU
    conv = nn.Conv2d(Cin, Cout, 1, bias=True).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
        with ops.kernel_trace() as tr:
            ya = ops.conv_act_eval(x, conv)
    assert ya is not None and _traced(tr) == [want], _traced(tr)
    y2 = torch.full_like(ya, float('nan'))
    _abi_forward(x, pk, b, y2, shape, 'f32', act=1)
    assert not torch.isnan(y2).any() and torch.equal(ya, y2)
    err = _rel(ya, torch.nn.functional.silu(ref_b))
    assert err < 1e-5, f'SiLU {err:.2e}'


# ------------------------------------------------------------------------------------------------ 3. weight gradient
W1_SHAPES = {24: (1, 4, 1), 40: (2, 2, 2), 72: (4, 1, 4)}          # Cout -> (WVM, WVN, NT): w1_shape; each Cout leaves a ragged last output tile


def _w1_symbol(Cout, HW, op):
    wvm, wvn, nt = W1_SHAPES[Cout]
    return f'conv1x1_wgrad_lds_kernel<{3 if op == "f32" else 1}, {wvm}, {wvn}, {nt}, {2 if HW % 32 == 0 else 1}, {"true" if op == "planes" else "false"}>'


def _w1_slices(NI, Cin, Cout, H, W, op):
    """eas_conv1x1_wgrad_slices through the workspace query: slabs of Cout * Cin floats"""
    from eas_snn_amd import _lib
    nws = _lib.lib().eas_conv_wgrad_workspace_floats(NI, Cin, Cout, H, W, 1, 1, {'f32': 3, 'int': 1, 'planes': 2}[op])
    assert nws % (Cout * Cin) == 0
    return nws // (Cout * Cin)


def _wgrad_inputs(dev, NI, Cin, Cout, H, W, ints):
    g = torch.Generator().manual_seed(NI * 1000 + Cin * 13 + Cout + H * W + int(ints))
    x = torch.randint(0, 4, (NI, Cin, H, W), generator=g).float() if ints else torch.randn(NI, Cin, H, W, generator=g)
    gy = torch.randn(NI, Cout, H, W, generator=g)
    return x.to(dev), gy.to(dev)


def _wgrad(dev, NI, Cin, Cout, H, W, op, x, gy):
    """grad_w of the traced ``ops.conv_wgrad``; the instance, 'written everywhere' (slabs and gradient start as NaN) and 'same bits twice' are
    asserted here"""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    xt = 3 if op == 'f32' else 1
    sp = ops.to_planes(x) if op == 'planes' else None
    with ops.kernel_trace() as tr:
        gw = ops.conv_wgrad(x, gy, 1, 1, xt, sp)
    want = _w1_symbol(Cout, H * W, op)
    assert _traced(tr, 'conv1x1_wgrad') == [want], (_traced(tr, 'conv1x1_wgrad'), want)
    ns = _w1_slices(NI, Cin, Cout, H, W, op)
    ws = torch.full((ns * Cout * Cin,), float('nan'), device=dev)
    if op == 'planes':
        got = L.eas_conv_wgrad_planes_partial(ops.ptr(sp), ops.ptr(gy), ops.ptr(ws), NI, Cin, Cout, H, W, 1, 1, ops.stream())
    else:
        got = L.eas_conv_wgrad_partial(ops.ptr(x), ops.ptr(gy), ops.ptr(ws), NI, Cin, Cout, H, W, 1, 1, xt, ops.stream())
    assert got == ns, (got, ns)
    assert not torch.isnan(ws).any(), 'a slab has unwritten elements'
    gw2 = torch.full_like(gw, float('nan'))
    job = (_lib.EasWgradReduceJob * 1)(_lib.EasWgradReduceJob(ws.data_ptr(), gw2.data_ptr(), gw2.numel(), ns))
    assert L.eas_conv_wgrad_reduce_many(job, 1, ops.stream()) == 0
    assert not torch.isnan(gw2).any() and torch.equal(gw, gw2), 'two identical calls differ'
    return gw


def _wgrad_check(dev, NI, Cin, Cout, H, W, op):
    from eas_snn_amd import ops
    x, gy = _wgrad_inputs(dev, NI, Cin, Cout, H, W, op != 'f32')
    gw = _wgrad(dev, NI, Cin, Cout, H, W, op, x, gy)
    ref = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 1, 1), gy.double())
    err = _rel(gw, ref)
    assert err < 1e-5, f'{err:.2e}'
    if op == 'planes':
        assert torch.equal(gw, ops.conv_wgrad(x, gy, 1, 1, 1))
    return gw


@pytest.mark.parametrize('op', OPERANDS)
@pytest.mark.parametrize('H,W', [(6, 8), (8, 8)], ids=['hw48_ks1', 'hw64_ks2'])
@pytest.mark.parametrize('Cout', [24, 40, 72])
def test_wgrad_instances(dev, Cout, H, W, op):
    """3 block shapes x 2 chunk widths x 3 operand forms = the 18 instances; Cin = 40: a ragged second 32-channel tile of x; two images"""
    _wgrad_check(dev, 2, 40, Cout, H, W, op)


@pytest.mark.parametrize('op', OPERANDS)
@pytest.mark.parametrize('Cout', [24, 40, 72])
def test_wgrad_two_input_channel_blocks(dev, Cout, op):
    """Cin = 136: every block shape covers 128 input channels, so two input-channel blocks, the second with 8 channels"""
    _wgrad_check(dev, 2, 136, Cout, 6, 8, op)


@pytest.mark.parametrize('Cout', [24, 40, 72])
def test_wgrad_short_last_slice_across_images(dev, Cout):
    """NI = 3 and a slice count (asked of the library) that does not divide the chunk count: the last slice is short, and slices walk
    across an image boundary.  The first shape of a fixed candidate order with that property is taken, and the property is asserted."""
    NI, W, found = 3, 16, None
    for Cin in (136, 264, 520, 1032):
        for H in range(3, 96, 2):           # HW = 16 * H, H odd: 16-pixel chunks (KS = 1), H chunks per image
            ns = _w1_slices(NI, Cin, Cout, H, W, 'f32')
            per = -(-NI * H // ns) if ns > 0 else 0
            if ns > 1 and (NI * H) % per != 0 and H % per != 0:
                found = (Cin, H, ns, per)
                break
        if found:
            break
    assert found, 'no candidate shape has a short last slice that crosses an image boundary'
    Cin, H, ns, per = found
    chunks = NI * H
    assert (ns - 1) * per < chunks < ns * per, 'the last slice must be short'
    assert any((s * per) // H != (min(s * per + per, chunks) - 1) // H for s in range(ns)), 'a slice must walk across an image boundary'
    _wgrad_check(dev, NI, Cin, Cout, H, W, 'f32')


def test_wgrad_refusals(dev):
    """HW % 16 != 0 and spike planes with Cin % 8 != 0 have no 1x1 weight-gradient kernel: the query says 0, the launch answers
    EAS_ERR_UNSUPPORTED before anything runs, and ops.conv2d computes such a layer's grad_w on the library route"""
    import torch.nn as nn
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    EAS_ERR_UNSUPPORTED = -2
    NI, Cin, Cout, H, W = 2, 16, 24, 5, 7          # HW = 35
    x, gy = _wgrad_inputs(dev, NI, Cin, Cout, H, W, True)
    ws = torch.full((Cout * Cin,), SENT, device=dev)
    sp = torch.zeros((NI, Cin // 8, H * W, 8), dtype=torch.bfloat16, device=dev)          # (no conversion to planes for HW % 4 != 0; never read)
    # planes whose channel count is no multiple of 8 (HW = 48 would be fine): a planes buffer of two groups stands in for the 12 channels
    x12, gy12 = _wgrad_inputs(dev, NI, 12, Cout, 6, 8, True)
    sp16 = ops.to_planes(torch.cat([x12, torch.zeros(NI, 4, 6, 8, device=dev)], 1))
    before = L.eas_launch_counter()
    for xt in (3, 1, 2):
        assert L.eas_conv_wgrad_workspace_floats(NI, Cin, Cout, H, W, 1, 1, xt) == 0
    for xt in (3, 1):
        assert L.eas_conv_wgrad_partial(ops.ptr(x), ops.ptr(gy), ops.ptr(ws), NI, Cin, Cout, H, W, 1, 1, xt, ops.stream()) == EAS_ERR_UNSUPPORTED
    assert L.eas_conv_wgrad_planes_partial(ops.ptr(sp), ops.ptr(gy), ops.ptr(ws), NI, Cin, Cout, H, W, 1, 1, ops.stream()) == EAS_ERR_UNSUPPORTED
    assert L.eas_conv_wgrad_workspace_floats(NI, 12, Cout, 6, 8, 1, 1, 3) > 0          # (fp32 input: any channel count)
    assert L.eas_conv_wgrad_workspace_floats(NI, 12, Cout, 6, 8, 1, 1, 2) == 0
    assert L.eas_conv_wgrad_planes_partial(ops.ptr(sp16), ops.ptr(gy12), ops.ptr(ws), NI, 12, Cout, 6, 8, 1, 1, ops.stream()) == EAS_ERR_UNSUPPORTED
    assert L.eas_launch_counter() == before, 'a refused call launched a kernel'
    torch.cuda.synchronize()
    assert bool((ws == SENT).all())
    with pytest.raises(_lib.EasHipError):
        ops.conv_wgrad(x, gy, 1, 1, 3)
    # the layer itself: grad_w from the library convolution
    conv = nn.Conv2d(Cin, Cout, 1, bias=False).to(dev)
    xr = torch.randn(NI, Cin, H, W, generator=torch.Generator().manual_seed(5)).to(dev).requires_grad_(True)
    assert ops.conv_eligible(xr, conv) and not ops.conv_route(xr.shape, Cout, 1, 1, 3).wgrad
    with ops.kernel_trace() as tr:
        y = ops.conv2d(xr, conv)
        y.backward(gy)
    assert not _traced(tr, 'conv1x1_wgrad'), _traced(tr, 'conv1x1_wgrad')
    ref = torch.nn.grad.conv2d_weight(xr.detach().double(), (Cout, Cin, 1, 1), gy.double())
    err = _rel(conv.weight.grad, ref)
    assert err < 1e-5, f'{err:.2e}'


# ------------------------------------------------------------------------------------------------ 4. grouped launches
# name -> (instance, [(NI, Cin, Cout, H, W)] x 3).  Different Cin: the launch orders the problems by their channel loops, longest first.
# Ragged Cout everywhere; different MT inside a group: grid.y covers the widest problem, the blocks past a narrower one leave.
GROUP_CASES = {
    'tile21': ('conv1x1_group_kernel<3, 2, 1, false, 0, C1GeomCore>', [(20, 24, 72, 32, 40), (20, 8, 136, 16, 20), (20, 40, 72, 16, 19)]),
    'ragged41': ('conv1x1_group_kernel<3, 4, 1, true, 0, C1GeomCore>', [(20, 4, 136, 32, 40), (20, 13, 136, 16, 20), (20, 24, 264, 16, 19)]),
    'mixed': ('conv1x1_group_kernel<3, 1, 1, false, 0, C1GeomCore>', [(2, 8, 24, 16, 20), (2, 40, 120, 8, 10), (2, 24, 72, 5, 7)])}


def _launch_group(xs, pks, bs, ys, accumulate):
    """``ops_group._launch_conv_group`` with a per-problem ``accumulate``"""
    from eas_snn_amd import _lib, ops
    n = len(xs)
    arr = (_lib.EasConvProblem * n)()
    for i, q in enumerate(arr):
        q.x, q.packed_w, q.bias, q.y, q.stats = ops.ptr(xs[i]), ops.ptr(pks[i]), ops.ptr(bs[i]), ops.ptr(ys[i]), None
        q.NI, q.Cin, q.Cout, q.Hi, q.Wi = xs[i].shape[0], xs[i].shape[1], ys[i].shape[1], xs[i].shape[2], xs[i].shape[3]
        q.accumulate = int(accumulate[i])
    ops.check(_lib.lib().eas_conv_fwd_group(arr, n, 1, 3, ops.stream()), 'eas_conv_fwd_group')


@pytest.mark.parametrize('name', list(GROUP_CASES))
def test_grouped_launch(dev, name):
    """three problems in one grid: plain through ops_group._launch_conv_group into NaN-filled outputs, then the same group with a bias on
    one problem and ``accumulate`` on another whose y is pre-filled: fp64 (+ what y held before)"""
    from eas_snn_amd import ops
    from eas_snn_amd import ops_group as G
    want, probs = GROUP_CASES[name]
    g = torch.Generator().manual_seed(len(name) + probs[0][0])
    xs = [torch.randn(NI, Cin, H, W, generator=g).to(dev) for NI, Cin, Cout, H, W in probs]
    ws = [(torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5).to(dev) for NI, Cin, Cout, H, W in probs]
    bias = torch.randn(probs[2][2], generator=g).to(dev)
    pks = [ops.conv_pack_weights(w, 0) for w in ws]
    refs = [_conv64(x, w) for x, w in zip(xs, ws)]
    runs = []
    for _ in range(2):
        ys = [torch.full((p[0], p[2], p[3], p[4]), float('nan'), device=dev) for p in probs]
        with ops.kernel_trace() as tr:
            G._launch_conv_group(xs, pks, None, ys, None, 1)
        assert _traced(tr) == [want], _traced(tr)
        runs.append(ys)
    for i, (y, y2, ref) in enumerate(zip(*runs, refs)):
        assert not torch.isnan(y).any(), f'problem {i}: y has unwritten elements'
        assert torch.equal(y, y2), f'problem {i}: two identical calls differ'
        err = _rel(y, ref)
        assert err < 1e-5, f'problem {i}: {err:.2e}'
    # problem 1 adds to what its y holds, problem 2 carries a bias
    before = torch.randn(refs[1].shape, generator=g).to(dev)
    ys = [torch.full_like(runs[0][0], float('nan')), before.clone(), torch.full_like(runs[0][2], float('nan'))]
    with ops.kernel_trace() as tr:
        _launch_group(xs, pks, [None, None, bias], ys, [0, 1, 0])
    assert _traced(tr) == [want], _traced(tr)
    assert torch.equal(ys[0], runs[0][0])
    err = _rel(ys[1], refs[1] + before.double())
    assert err < 1e-5, f'accumulate: {err:.2e}'
    err = _rel(ys[2], refs[2] + bias.double().view(1, -1, 1, 1))
    assert err < 1e-5, f'bias: {err:.2e}'
