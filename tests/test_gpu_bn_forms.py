"""One BatchNorm-fused layer, whichever entry point carries it.

A BN + (P)LIF layer on a channel range of a convolution output runs through ``ops.bn_lif_multistep`` (one layer on its own tensor) or as
one half of ``ops.bn_lif_pair`` (``layer.fused_pair``: two layers on the two ranges of ONE tensor); a BN + SiLU layer through
``ops.bn_silu``, ``ops.bn_silu_pair`` or as one problem of ``ops_group.bn_silu_group``.  The forms launch the same kernels on the same
numbers, so everything they compute is compared bit for bit -- at the smallest shapes with a non-zero channel offset (ranges 8 | 16 of 24
channels), gradients that arrive as non-contiguous channel slices, in-place concatenation and whole groups of 8 channels as spike planes.
Public entry points only: the file passes unchanged before and after a change of the operator layer behind them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, N, CA, CB, H, W = 2, 2, 8, 16, 4, 6
EPS, MOMENTUM = 1e-3, 0.03


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


def _assert_same(ref, got, what):
    """every quantity of ``got`` bit-identical to ``ref``; all differences are printed before the first one fails the test"""
    worst = {k: float((got[k].double() - ref[k].double()).abs().max()) for k in ref if not torch.equal(ref[k], got[k])}
    for k, d in worst.items():
        print(f'{what}: {k} differs, max |difference| {d:.3e} (max |reference| {float(ref[k].abs().max()):.3e})')
    assert not worst, f'{what}: not bit-identical: {sorted(worst)}'


def _fill_bn(bn, gamma, beta):
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    return bn


def test_bn_lif_single_and_pair_are_bit_identical(dev):
    """``bn_lif_multistep`` on contiguous copies of the two channel ranges against ``bn_lif_pair`` on the whole tensor; into fresh outputs,
    into the halves of a concatenation buffer (``join_channels``), and both again with the output as bf16 spike planes.  Training-mode
    statistics, PLIF with a learnable w; backward from one random gradient of the concatenation.  Spikes, final potentials, running
    statistics and the gradients of y, gamma, beta and w: bit-identical between all eight runs."""
    from eas_snn_amd import ops
    from spikingjelly.activation_based import layer, neuron, surrogate
    g = torch.Generator().manual_seed(3)
    y12 = (torch.randn(T, N, CA + CB, H, W, generator=g) * 1.5 + 0.3).to(dev)          # scaled so that neurons fire
    gamma, beta = (torch.rand(CA + CB, generator=g) + 0.6).to(dev), (torch.rand(CA + CB, generator=g) * 0.6 - 0.1).to(dev)
    gcat = torch.randn(T, N, CA + CB, H, W, generator=g).to(dev)
    ranges = ((0, CA, 2.0), (CA, CB, 3.0))

    def run(pair, cat, planes):
        bns = [_fill_bn(layer.BatchNorm2d(c, eps=EPS, momentum=MOMENTUM, step_mode='m').to(dev).train(), gamma[c0:c0 + c], beta[c0:c0 + c])
               for c0, c, _ in ranges]
        nodes = [neuron.ParametricLIFNode(init_tau=tau, decay_input=False, v_reset=None, surrogate_function=surrogate.ATan(2.0),
                                          step_mode='m').to(dev) for _, _, tau in ranges]
        buf = sp_buf = None
        if cat:
            buf = ops.ghost((T, N, CA + CB, H, W), dev) if planes else torch.empty(T, N, CA + CB, H, W, device=dev)
            sp_buf = ops.new_planes(T, N, CA + CB, H, W, dev) if planes else None
        cats = [(buf, c0, sp_buf) if cat else None for c0, _, _ in ranges]
        with ops.state_writeback_scope(True):
            if pair:
                y = y12.clone().requires_grad_(True)
                outs = layer.fused_pair(bns[0], nodes[0], bns[1], nodes[1], y, cat_a=cats[0], cat_b=cats[1], planes_a=planes, planes_b=planes)
                vs = [nd.v for nd in nodes]
            else:
                ys = [y12[:, :, c0:c0 + c].contiguous().requires_grad_(True) for c0, c, _ in ranges]
                outs, vs = [], []
                for yc, bn, nd, ct in zip(ys, bns, nodes, cats):
                    a = nd.lif_args()
                    s, v, _ = ops.bn_lif_multistep(yc, bn.weight, bn.bias, bn.running_mean, bn.running_var, True, MOMENTUM, EPS, None, a['w'],
                                                   a['k_const'], a['v_th'], a['v_reset'], a['flags'], a['surrogate'], a['alpha'], write_v=True,
                                                   cat=ct, planes=planes)
                    outs.append(ops.mark_small_int(s))
                    vs.append(v)
        assert all((ops.planes_of(s) is not None) == planes for s in outs)
        if cat:
            full = ops.join_channels(buf, *outs, sp_buf=sp_buf)
            assert (ops.planes_of(full) is not None) == planes
            full.backward(gcat)
        else:
            torch.autograd.backward(list(outs), [gcat[:, :, c0:c0 + c] for c0, c, _ in ranges])      # non-contiguous channel slices
        with torch.no_grad():
            spikes = ops.dense(full) if cat else torch.cat([ops.dense(s) for s in outs], 2)
        res = dict(spikes=spikes.detach().clone(), grad_y=y.grad if pair else torch.cat([yc.grad for yc in ys], 2))
        for name, bn, nd, v in zip('ab', bns, nodes, vs):
            res.update({f'v_{name}': v, f'running_mean_{name}': bn.running_mean, f'running_var_{name}': bn.running_var,
                        f'grad_gamma_{name}': bn.weight.grad, f'grad_beta_{name}': bn.bias.grad, f'grad_w_{name}': nd.w.grad})
        return res

    ref = run(False, False, False)
    rate = float(ref['spikes'].mean())
    assert 0.02 < rate < 0.98, f'firing rate {rate}: the comparison needs neurons that fire and neurons that do not'
    assert all(float(ref[k].abs().max()) > 0 for k in ref), 'a compared quantity is all zero'
    for pair in (False, True):
        for cat in (False, True):
            for planes in (False, True):
                if pair or cat or planes:
                    _assert_same(ref, run(pair, cat, planes), f'BN+LIF pair={pair} cat={cat} planes={planes}')


def test_bn_silu_single_pair_and_group_are_bit_identical(dev):
    """``bn_silu`` on contiguous copies of the two channel ranges, ``bn_silu_pair`` on the whole tensor and ``bn_silu_group`` with the two
    ranges as two layers of one output, all behind the same 1x1 ``conv_group`` of 8 -> 24 channels; single and pair also into the halves of
    a concatenation buffer.  Outputs, running statistics and the gradients of y, gamma and beta: bit-identical.  (The grouped form takes
    its statistics from that convolution's tile sums and reduces its parameter gradients in its own kernel: other summation orders, which
    on other inputs can differ from the per-layer kernels in the last bit.  The inputs here are fixed by their seed, and on them the three
    forms agree bit for bit.)"""
    from eas_snn_amd import ops, ops_group
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, 8, H, W, generator=g).to(dev)
    conv = torch.nn.Conv2d(8, CA + CB, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(CA + CB, 8, 1, 1, generator=g) / 8 ** 0.5)
    conv.to(dev)
    gamma, beta = (torch.rand(CA + CB, generator=g) + 0.5).to(dev), (torch.randn(CA + CB, generator=g) * 0.3).to(dev)
    gcat = torch.randn(N, CA + CB, H, W, generator=g).to(dev)
    ranges = ((0, CA), (CA, CB))

    def run(form, cat):
        bns = [_fill_bn(torch.nn.BatchNorm2d(c, eps=EPS, momentum=MOMENTUM).to(dev).train(), gamma[c0:c0 + c], beta[c0:c0 + c]) for c0, c in ranges]
        with torch.no_grad():
            ys, stats = ops_group.conv_group([x], [conv], 1, True)
        y = ys[0].requires_grad_(True)
        buf = torch.empty(N, CA + CB, H, W, device=dev) if cat else None
        cats = [(buf, c0) if cat else None for c0, _ in ranges]
        if form == 'single':
            parts = [y.detach()[:, c0:c0 + c].contiguous().requires_grad_(True) for c0, c in ranges]
            outs = [ops.bn_silu(p, bn, cat=ct) for p, bn, ct in zip(parts, bns, cats)]
        elif form == 'pair':
            outs = ops.bn_silu_pair(y, bns[0], bns[1], cat_a=cats[0], cat_b=cats[1])
        else:
            outs = ops_group.bn_silu_group([y], stats, [(0, c0, bn) for (c0, _), bn in zip(ranges, bns)])
        if cat:
            full = ops.join_channels(buf, *outs)
            full.backward(gcat)
        else:
            torch.autograd.backward(list(outs), [gcat[:, c0:c0 + c] for c0, c in ranges])            # non-contiguous channel slices
        res = dict(out=(full if cat else torch.cat(list(outs), 1)).detach().clone(),
                   grad_y=torch.cat([p.grad for p in parts], 1) if form == 'single' else y.grad)
        for name, bn in zip('ab', bns):
            res.update({f'running_mean_{name}': bn.running_mean, f'running_var_{name}': bn.running_var,
                        f'grad_gamma_{name}': bn.weight.grad, f'grad_beta_{name}': bn.bias.grad})
        return res

    ref = run('single', False)
    assert all(float(ref[k].abs().max()) > 0 for k in ref), 'a compared quantity is all zero'
    for form, cat in (('pair', False), ('single', True), ('pair', True), ('group', False)):
        _assert_same(ref, run(form, cat), f'BN+SiLU {form} cat={cat}')


def test_bn_pending_statistics_refused_alike(dev):
    """The three forward entry points that finalize pending statistics themselves (``EasBnPending``: eas_bn_lif_fwd_ex, eas_bn_silu_fwd_ex,
    eas_bn_silu_fwd_group) accept and refuse the same structs: each invalid one is EAS_ERR_INVALID_ARG from all three without a launch,
    the valid one runs in all three.  Through the C ABI (the operator layer never builds an invalid struct)."""
    import ctypes
    from eas_snn_amd import _lib
    L, st = _lib.lib(), _lib.stream()
    Tn, Nn, Cn, HW = 2, 2, 8, 24
    y = torch.randn(Tn, Nn, Cn, HW, device=dev)
    gamma, beta = torch.rand(Cn, device=dev) + 0.5, torch.randn(Cn, device=dev)
    mean, invstd = torch.empty(Cn, device=dev), torch.empty(Cn, device=dev)
    rmean, rvar = torch.zeros(Cn, device=dev), torch.ones(Cn, device=dev)
    out = torch.empty_like(y)
    stats = {}                      # images -> (workspace, chunks) of the statistics pass: T * N images for the neuron layer, N for SiLU
    for tn in (Tn * Nn, Nn):
        ws = torch.empty(L.eas_bn_workspace_doubles(Cn), dtype=torch.float64, device=dev)
        stats[tn] = ws, L.eas_bn_stats_partial(y.data_ptr(), 0, tn, Cn, HW, ws.data_ptr(), st)
        assert stats[tn][1] >= 1

    def pending(tn, **change):
        f = dict(partial=stats[tn][0].data_ptr(), chunks=stats[tn][1], replicas=1, count=float(tn * HW), eps=EPS, momentum=MOMENTUM,
                 running_mean=rmean.data_ptr(), running_var=rvar.data_ptr(), pitch=0)
        f.update(change)
        return _lib.EasBnPending(**f)

    def lif(tn, **change):
        return L.eas_bn_lif_fwd_ex(y.data_ptr(), 0, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, None, None, 0.5,
                                   1.0, 0.0, 0, out.data_ptr(), None, Tn, Nn, Cn, HW, 0, ctypes.byref(pending(tn, **change)), None, 0, None,
                                   None, 0, st)

    def silu(tn, **change):
        return L.eas_bn_silu_fwd_ex(y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), Nn, Cn,
                                    HW, ctypes.byref(pending(tn, **change)), 0, 0, st)

    def silu_group(tn, **change):
        arr = (_lib.EasBnSiluFwdProblem * 1)(_lib.EasBnSiluFwdProblem(y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                                                      beta.data_ptr(), out.data_ptr(), Nn, Cn, HW, 0, 0, pending(tn, **change)))
        return L.eas_bn_silu_fwd_group(arr, 1, st)

    invalid = {'chunks = 0': dict(chunks=0), 'chunks > pitch': dict(chunks=5, pitch=4), 'chunks > default pitch': dict(chunks=65),
               'negative pitch': dict(pitch=-1), 'count = 0.5': dict(count=0.5), 'replicas = 0': dict(replicas=0),
               'running_mean only': dict(running_var=None), 'running_var only': dict(running_mean=None)}
    INVALID_ARG = -1                # include/eas_hip.h EAS_ERR_INVALID_ARG
    for entry, tn in ((lif, Tn * Nn), (silu, Nn), (silu_group, Nn)):
        for what, change in invalid.items():
            before = L.eas_launch_counter()
            rc = entry(tn, **change)
            assert rc == INVALID_ARG, f'{entry.__name__}: {what}: status {rc}'
            assert L.eas_launch_counter() == before, f'{entry.__name__}: {what}: a refused call launched a kernel'
        before = L.eas_launch_counter()
        assert entry(tn) == 0, f'{entry.__name__}: the valid struct is refused'
        assert L.eas_launch_counter() == before + 1
        torch.cuda.synchronize()
        assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(invstd).all())
