"""The 3x3 convolution kernels (conv_mfma_body.h, conv_mfma.hip, conv_s2d.hip, conv_group.hip): every instance the default library launches
anywhere in the search box of tests/conv3x3_cases.py, in every run-time form, at the smallest box shape that reaches it, against fp64.

The rows come from tests/conv3x3_cases.py; tests/test_cpu_conv3x3_plan.py proves without a GPU that every row lands on the instance and
run-time form it promises and that the box holds nothing else.  Every case here (1) runs under ``ops.kernel_trace()`` and asserts the traced
symbol, cut down by ``test_gpu_conv1x1_instances._short``, carries exactly the promised template arguments; (2) writes into NaN-filled
outputs and finds no NaN left; (3) compares with ``conv2d`` / ``conv2d_input`` in double on the device, max |difference| / max |reference|
< 1e-5 (the project's bar); (4) makes the same call twice -- through the operator, then on the C ABI into the NaN-filled output -- and
requires the same bits.

Instances and the cases that launch them:

plain forward, LM = 0 -- test_forward[row-operand], one case per row of CASES (fp32 three terms; one-term rows twice: fp32 small integers
and spike planes, the planes result bit-identical to the fp32 one):
  conv_fwd_mfma_kernel<9, S, XT, 1, WN, WVM, WVN, 16, VEC, NIT, PL, 0>, (WVM, WVN, WN) = TILES[candidate]
    S = 1, XT = 3, VEC 4: candidates 0 1 2 4 5 6 7 8 10 11 12 13; S = 1, XT = 1 (fp32 and planes), VEC 4: 0 3 4 5 6 10 11 12 13
    S = 2, XT = 3, VEC 4: 2 6 8 9 11 12 13;                      S = 2, XT = 1 (fp32 and planes), VEC 4: 0 1 6 7 10 11 12 13
    VEC 2 (either stride, all three operand forms): 11 12 13                                         -- 71 of the 168 instances
  run-time forms per instance (single-buffered patch, 2 / 4 column parts, several whole images per tile, a short last tile): the key of
  the row; edges (Cin 8 / 24 / 40 / 136, ragged and idle channel tiles, odd maps, tiles no multiple of 32 pixels): the row's comment
  every stride-1 three-term row runs its instance a second time as an input gradient (weights packed with mode 1) against conv2d_input
  left out: conv3x3_cases.LEFT_OUT, 97 instances no shape of the box reaches, each with the reason; eight column parts (no box shape)
  bias, statistics and SiLU epilogues (run-time branches): test_epilogues, one shape per (stride, candidate)

stride-2 input gradient -- test_stride2_input_gradient, S2D_CASES: conv_dgrad_s2c_kernel<WN, WVM, WVN, VEC>
  <2, 2, 2, 2>, <2, 1, 4, 4 | 2 | 1>, <1, 4, 1, 2>, <1, 2, 2, 2>: 6 of 21; the rest: conv3x3_cases.S2D_LEFT_OUT

grouped -- test_grouped_launch, GROUP_CASES: conv3x3_group_kernel<3, WN, WVM, WVN, 2, 0, ConvGeomCore>, all four tiles

The fused forms stay with their bit-identity tests in tests/test_gpu_kernels.py, which tie them to the unfused composition whose plain tiles
the cases here tie to fp64.  From the kernel traces of those tests (template arguments <9, S, XT, 1, WN, WVM, WVN, 16, VEC, NIT, PL, LM>):
  fused eval step, LM = 1 (dispatch_tile_lif, time-major, planes) -- test_fused_eval_step_is_bit_identical_to_conv_then_bn_lif:
    <9, 1, 1, 1, 3, 1, 4, 16, 2, 2, true, 1>, <9, 1, 1, 1, 3, 1, 4, 16, 4, 2, true, 1>, <9, 1, 1, 1, 3, 2, 2, 16, 4, 2, true, 1>,
    <9, 1, 1, 1, 5, 2, 2, 16, 4, 2, true, 1>, <9, 1, 1, 1, 6, 2, 2, 16, 2, 2, true, 1>, <9, 2, 1, 1, 3, 2, 2, 16, 4, 2, true, 1>,
    <9, 2, 1, 1, 5, 2, 2, 16, 4, 2, true, 1>; no LM = 2 instance (one frame set shared by all steps) is launched there
  BatchNorm + activation epilogue, LM = 3 (dispatch_tile itself: the tile eas_conv_fwd_plan names for x_terms 3) --
  test_fused_real_valued_eval_block_is_bit_identical_to_conv_then_bn_silu:
    <9, 1, 3, 1, 3, 2, 2, 16, 4, 2, false, 3>, <9, 1, 3, 1, 3, 4, 1, 16, 2, 2, false, 3>, <9, 1, 3, 1, 5, 4, 1, 16, 4, 2, false, 3>,
    <9, 2, 3, 1, 3, 2, 2, 16, 4, 2, false, 3>, <9, 2, 3, 1, 3, 4, 1, 16, 4, 2, false, 3>
  grouped LM = 3 (conv3x3_group_kernel<3, .., 3, ConvGeomBna>): test_grouped_bn_silu_forward_backward_vs_fp64, which runs outside a trace."""
import functools

import pytest
import torch

import conv3x3_cases as K
from test_gpu_conv1x1_instances import _rel, _short, _traced

pytestmark = pytest.mark.gpu

SENT = 12345.0
EAS_ERR_UNSUPPORTED = -2
_WORST = {}          # family -> largest relative error seen (printed when the module is done)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    yield torch.device('cuda:0')
    _case.cache_clear()
    print('\nconv3x3 instances, largest relative error per family:', {k: f'{v:.2e}' for k, v in sorted(_WORST.items())})


def _bar(family, got, ref, what=''):
    err = _rel(got, ref)
    _WORST[family] = max(_WORST.get(family, 0.0), err)
    assert err < 1e-5, f'{what} {err:.2e}'


def _conv64(x, w, stride, b=None):
    """fp64 3x3 convolution, padding 1, on the device (ATen: no library of ours involved)"""
    return torch.nn.functional.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=stride, padding=1)


@functools.lru_cache(maxsize=6)
def _case(shape, stride, ints):
    """inputs of one shape and their fp64 convolution, made once and shared by the cases that read them (nothing writes to them): randn for
    three terms, small integers 0..3 for one term and planes, weights randn / sqrt(9 Cin) -- as test_gpu_conv1x1_instances._case"""
    NI, Cin, Cout, H, W = shape
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(NI * 1009 + Cin * 31 + Cout * 7 + H * W + int(ints) + 2 * stride)
    x = torch.randint(0, 4, (NI, Cin, H, W), generator=g, device=dev).float() if ints else torch.randn(NI, Cin, H, W, generator=g, device=dev)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, device=dev) / (9 * Cin) ** 0.5
    b = torch.randn(Cout, generator=g, device=dev)
    return x, w, b, _conv64(x, w, stride)


def _planes(x):
    """spike planes bf16 [NI][Cin / 8][H * W][8] of small integers; ops.to_planes where it exists (H * W % 4 == 0), else by permutation"""
    from eas_snn_amd import ops
    NI, Cin, H, W = x.shape
    if (H * W) % 4 == 0:
        return ops.to_planes(x)
    return x.view(NI, Cin // 8, 8, H * W).permute(0, 1, 3, 2).contiguous().to(torch.bfloat16)


def _abi_forward(xin, pk, bias, y, shape, stride, op, act=0, stats=None, nb=0):
    """the C-ABI call ``ops.conv_fwd_packed`` makes for this operand form, writing into the caller's ``y``"""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    NI, Cin, Cout, H, W = shape
    p, xt = ops.ptr, (3 if op == 'f32' else 1)
    if op == 'planes':
        assert not act
        rc = L.eas_conv_fwd_planes(p(xin), p(pk), p(bias), p(y), NI, Cin, Cout, H, W, 3, stride, p(stats), nb, ops.stream())
    elif act:
        rc = L.eas_conv_fwd_act(p(xin), p(pk), p(bias), p(y), NI, Cin, Cout, H, W, 3, stride, xt, act, None, ops.stream())
    elif stats is not None:
        rc = L.eas_conv_fwd_stats(p(xin), p(pk), p(y), NI, Cin, Cout, H, W, 3, stride, xt, None, p(stats), nb, ops.stream())
    else:
        rc = L.eas_conv_fwd(p(xin), p(pk), p(bias), p(y), NI, Cin, Cout, H, W, 3, stride, xt, None, ops.stream())
    assert rc == 0, rc


def _forward(shape, stride, op, want, x, pk, bias=None, act=0):
    """y of the traced operator call; the instance, 'written everywhere' and 'same bits twice' are asserted here"""
    from eas_snn_amd import ops
    sp = _planes(x) if op == 'planes' else None
    with ops.kernel_trace() as tr:
        y = ops.conv_fwd_packed(x, pk, bias, shape[2], 3, stride, 3 if op == 'f32' else 1, sp, act=act)
    assert _traced(tr, 'conv_fwd_mfma') == [want], (shape, op, _traced(tr, 'conv_fwd_mfma'), want)
    y2 = torch.full_like(y, float('nan'))
    _abi_forward(sp if op == 'planes' else x, pk, bias, y2, shape, stride, op, act=act)
    assert not torch.isnan(y2).any(), 'y has unwritten elements'
    assert torch.equal(y, y2), 'two identical calls differ'
    return y


# ------------------------------------------------------------------------------------------------ 1. plain forward, LM = 0
FORWARD = [(key, shape, op) for key, shape in K.CASES for op in (('f32',) if key[1] == 3 else ('int', 'planes'))]
_fwd_id = lambda c: 's{}t{}v{}c{}-{}{}{}{}-{}-{}'.format(*c[0], 'x'.join(map(str, c[1])), c[2])


@pytest.mark.parametrize('case', FORWARD, ids=_fwd_id)
def test_forward(dev, case):
    from eas_snn_amd import ops
    key, shape, op = case
    s, vec, cand = key[0], key[2], key[3]
    NI, Cin, Cout, H, W = shape
    want = K.fwd_symbol(s, op, vec, cand)
    x, w, _, y64 = _case(shape, s, op != 'f32')
    pk = ops.conv_pack_weights(w, 0)
    y = _forward(shape, s, op, want, x, pk)
    _bar(f'forward stride {s} {"three terms" if op == "f32" else "one term"}', y, y64)
    if op == 'planes':          # the same products in the same order as the one-term fp32 form
        assert torch.equal(y, ops.conv_fwd_packed(x, pk, None, Cout, 3, s, 1))
    if op == 'f32' and s == 1:          # the same instance as an input gradient: grad_y in, the weight of the Cout -> Cin convolution packed with mode 1
        gy = x
        v = torch.randn(Cin, Cout, 3, 3, generator=torch.Generator(device=dev).manual_seed(Cin + Cout), device=dev) / (9 * Cin) ** 0.5
        with ops.kernel_trace() as tr:
            gx = ops.conv_fwd_packed(gy, ops.conv_pack_weights(v, 1), None, Cout, 3, 1, 3)
        assert _traced(tr, 'conv_fwd_mfma') == [want], _traced(tr, 'conv_fwd_mfma')
        ref = torch.nn.grad.conv2d_input((NI, Cout, H, W), v.double(), gy.double(), padding=1)
        _bar('input gradient stride 1', gx, ref, 'input gradient')
    assert not ops.tag_violation(dev)


# one row per (stride, candidate): three terms where the tile has such a row, the smallest
def _epilogue_rows():
    size = lambda r: r[1][0] * (r[1][1] + r[1][2]) * r[1][3] * r[1][4]
    best = {}
    for key, shape in K.CASES:
        k = (key[0], key[3])
        rank = (key[1] != 3, size((key, shape)))
        if k not in best or rank < best[k][0]:
            best[k] = (rank, key, shape)
    return [(key, shape) for _, key, shape in (best[k] for k in sorted(best))]


@pytest.mark.parametrize('row', _epilogue_rows(), ids=lambda r: 's{}c{}-{}'.format(r[0][0], r[0][3], 'x'.join(map(str, r[1]))))
def test_epilogues(dev, row):
    """bias, BatchNorm statistics and SiLU in the epilogue of every tile of both strides (run-time branches of the plain instances)"""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    key, shape = row
    s, terms, vec, cand = key[:4]
    NI, Cin, Cout, H, W = shape
    op = 'f32' if terms == 3 else 'int'
    x, w, b, y64 = _case(shape, s, op != 'f32')
    want = K.fwd_symbol(s, op, vec, cand)
    pk = ops.conv_pack_weights(w, 0)
    plain = _forward(shape, s, op, want, x, pk)
    # ---- bias
    yb = _forward(shape, s, op, want, x, pk, bias=b)
    ref_b = y64 + b.double().view(1, -1, 1, 1)
    _bar('epilogues', yb, ref_b, 'bias')
    # ---- statistics: y as the plain call, partial sums = the fp64 sums of that y (the bars of test_conv_epilogue_statistics)
    xt = 3 if op == 'f32' else 1
    nb = L.eas_conv_fwd_stats_blocks(NI, Cin, Cout, H, W, 3, s, xt)
    assert nb > 0
    runs = []
    for _ in range(2):
        y2 = torch.full_like(plain, float('nan'))
        st = torch.full((Cout * nb * 2,), float('nan'), dtype=torch.float64, device=dev)
        with ops.kernel_trace() as tr:
            _abi_forward(x, pk, None, y2, shape, s, op, stats=st, nb=nb)
        assert _traced(tr, 'conv_fwd_mfma') == [want], _traced(tr, 'conv_fwd_mfma')
        assert torch.equal(y2, plain) and torch.isfinite(st).all(), 'statistics epilogue: unwritten outputs or partial sums'
        runs.append(st)
    assert torch.equal(*runs), 'two identical calls differ'
    got = runs[0].view(Cout, nb, 2).sum(1)
    p64 = plain.double()
    ssum, ssq = p64.sum((0, 2, 3)), (p64 * p64).sum((0, 2, 3))
    assert float(((got[:, 0] - ssum).abs() / (p64.abs().sum((0, 2, 3)) + 1e-30)).max()) < 3e-7
    assert float(((got[:, 1] - ssq).abs() / (ssq + 1e-30)).max()) < 3e-7
    # ---- SiLU
    ya = _forward(shape, s, op, want, x, pk, bias=b, act=1)
    _bar('epilogues', ya, torch.nn.functional.silu(ref_b), 'SiLU')


# ------------------------------------------------------------------------------------------------ 2. stride-2 input gradient
@pytest.mark.parametrize('row', K.S2D_CASES, ids=lambda r: 'c{}v{}-{}{}{}-{}'.format(*r[0], 'x'.join(map(str, r[1]))))
def test_stride2_input_gradient(dev, row):
    """the checks of test_stride2_input_gradient_all_parity_classes_in_one_tile (NaN-filled grad_x, fp64 conv2d_input, the 4-byte-aligned
    view) on every reachable instance and tile form, with the symbol and the same bits from two calls"""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    key, (NI, Cin, Cout, H, W) = row
    want = K.s2d_symbol(key[0], key[1])
    g = torch.Generator().manual_seed(NI * 100 + Cin + H)
    Ho, Wo = K.out_size(H, W, 2)
    gy = torch.randn(NI, Cout, Ho, Wo, generator=g).to(dev)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).to(dev)
    pk = ops.conv_pack_weights(w, 2)
    outs = []
    for _ in range(2):
        gx = torch.full((NI, Cin, H, W), float('nan'), device=dev)
        with ops.kernel_trace() as tr:
            ops.check(L.eas_conv_dgrad_s2(ops.ptr(gy), ops.ptr(pk), ops.ptr(gx), NI, Cin, Cout, H, W, ops.stream()), 'eas_conv_dgrad_s2')
        assert _traced(tr, 'conv_dgrad_s2c') == [want], (_traced(tr, 'conv_dgrad_s2c'), want)
        assert not torch.isnan(gx).any(), 'grad_x has unwritten elements'
        outs.append(gx)
    assert torch.equal(*outs), 'two identical calls differ'
    ref = torch.nn.grad.conv2d_input((NI, Cin, H, W), w.double(), gy.double(), stride=2, padding=1)
    _bar('stride-2 input gradient', outs[0], ref)
    # a view that is only 4-byte aligned: the epilogue falls back to 4-byte stores
    buf = torch.full((outs[0].numel() + 1,), float('nan'), device=dev)
    gx2 = buf[1:].view_as(outs[0])
    ops.check(L.eas_conv_dgrad_s2(ops.ptr(gy), ops.ptr(pk), ops.ptr(gx2), NI, Cin, Cout, H, W, ops.stream()), 'eas_conv_dgrad_s2')
    assert torch.equal(gx2, outs[0]), 'the 4-byte store path differs'
    assert bool(torch.isnan(buf[0])), 'the element in front of the view was written'


# ------------------------------------------------------------------------------------------------ 3. grouped launches
@pytest.mark.parametrize('name', list(K.GROUP_CASES))
def test_grouped_launch(dev, name):
    """three problems of different map size and Cin in one grid, through ops_group._launch_conv_group into NaN-filled outputs, the last
    problem with a bias: symbol, no NaN, fp64 per problem, the same bits twice"""
    from eas_snn_amd import ops
    from eas_snn_amd import ops_group as G
    cand, probs, _ = K.GROUP_CASES[name]
    want = K.group_symbol(cand)
    g = torch.Generator().manual_seed(len(name) + probs[0][0] + cand)
    xs = [torch.randn(NI, Cin, H, W, generator=g).to(dev) for NI, Cin, Cout, H, W in probs]
    ws = [(torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).to(dev) for NI, Cin, Cout, H, W in probs]
    bias = torch.randn(probs[2][2], generator=g).to(dev)
    pks = [ops.conv_pack_weights(w, 0) for w in ws]
    refs = [_conv64(x, w, 1) for x, w in zip(xs, ws)]
    refs[2] = refs[2] + bias.double().view(1, -1, 1, 1)
    runs = []
    for _ in range(2):
        ys = [torch.full((p[0], p[2], p[3], p[4]), float('nan'), device=dev) for p in probs]
        with ops.kernel_trace() as tr:
            G._launch_conv_group(xs, pks, [None, None, bias], ys, None, 3)
        assert _traced(tr, 'conv3x3_group') == [want], (_traced(tr, 'conv3x3_group'), want)
        runs.append(ys)
    for i, (y, y2, ref) in enumerate(zip(*runs, refs)):
        assert not torch.isnan(y).any(), f'problem {i}: y has unwritten elements'
        assert torch.equal(y, y2), f'problem {i}: two identical calls differ'
        _bar('grouped', y, ref, f'problem {i}')


# ------------------------------------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize('geom', K.REFUSED, ids=lambda g: 'x'.join(map(str, g)))
def test_refusals(dev, geom):
    """Cin % 8 != 0, an odd Wi and rows no tile fits: EAS_ERR_UNSUPPORTED from every entry point of the forward, the launch counter does
    not move and a sentinel-filled y is untouched"""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    NI, Cin, Cout, H, W, s = geom
    Ho, Wo = K.out_size(H, W, s)
    x = torch.randint(0, 2, (NI, Cin, H, W), device=dev).float()
    sp = torch.zeros((NI, (Cin + 7) // 8, H * W, 8), dtype=torch.bfloat16, device=dev)          # (never read)
    pk = ops.conv_pack_weights(torch.randn(Cout, Cin, 3, 3, device=dev), 0)
    y = torch.full((NI, Cout, Ho, Wo), SENT, device=dev)
    st = torch.full((Cout * 8 * 2,), SENT, dtype=torch.float64, device=dev)
    p = ops.ptr
    torch.cuda.synchronize()
    before = L.eas_launch_counter()
    for xt in (3, 1):
        assert L.eas_conv_fwd(p(x), p(pk), None, p(y), NI, Cin, Cout, H, W, 3, s, xt, None, ops.stream()) == EAS_ERR_UNSUPPORTED
        assert L.eas_conv_fwd_act(p(x), p(pk), None, p(y), NI, Cin, Cout, H, W, 3, s, xt, 1, None, ops.stream()) == EAS_ERR_UNSUPPORTED
        assert L.eas_conv_fwd_stats(p(x), p(pk), p(y), NI, Cin, Cout, H, W, 3, s, xt, None, p(st), 8, ops.stream()) == EAS_ERR_UNSUPPORTED
    assert L.eas_conv_fwd_planes(p(sp), p(pk), None, p(y), NI, Cin, Cout, H, W, 3, s, None, 0, ops.stream()) == EAS_ERR_UNSUPPORTED
    assert L.eas_launch_counter() == before, 'a refused call launched a kernel'
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and bool((st == SENT).all())
