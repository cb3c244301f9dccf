"""CPU-only tests of the two pure rules of the BatchNorm-fused operator layer (eas_snn_amd/ops_bn.py): which gradients the kernels may
read in place as a channel slice of a wider tensor, and what a BatchNorm module does in one call (the state every fused form hands to
the kernels)."""
import pytest
import torch

from eas_snn_amd import _lib, ops
from spikingjelly.activation_based import layer, neuron, surrogate


def test_channel_slice_rule():
    for shape in ((2, 3, 24, 4, 6), (3, 24, 4, 6)):
        buf = torch.zeros(shape)
        assert ops._channel_slice(buf, 24) == 24                                   # contiguous: its own channel count
        assert ops._channel_slice(buf.narrow(-3, 8, 16), 16) == 24                 # channels 8..24 of 24
        assert ops._channel_slice(buf.narrow(-1, 0, 4), 24) == 0                   # a slice along W
        assert ops._channel_slice(buf.narrow(-2, 1, 2), 24) == 0                   # a slice along H
        assert ops._channel_slice(buf.transpose(-1, -2), 24) == 0
        assert ops._channel_slice(buf.double(), 24) == 0
        assert ops._channel_slice(buf.double().narrow(-3, 8, 16), 16) == 0
    buf = torch.zeros(2, 24, 3, 3)
    assert buf.data_ptr() % 16 == 0 and ops._channel_slice(buf.narrow(1, 1, 16), 16) == 0      # starts 36 bytes in: no 16-byte loads
    assert ops._channel_slice(buf.narrow(1, 4, 16), 16) == 24                                  # 144 bytes in
    assert ops._channel_slice(torch.zeros(2, 3, 24, 4, 6).narrow(1, 0, 2), 24) == 0            # 5-D along N: T stride is not N * pitch
    assert ops._channel_slice(torch.zeros(24, 4, 6).narrow(0, 8, 16), 16) == 0                 # neither 4-D nor 5-D


@pytest.mark.parametrize('mode', ['train', 'eval', 'no_running_stats', 'eval_momentum_none'])
def test_bn_state(mode, monkeypatch):
    kw = dict(no_running_stats=dict(track_running_stats=False), eval_momentum_none=dict(momentum=None)).get(mode, {})
    train = mode in ('train', 'no_running_stats')

    def make(c=8):
        return layer.BatchNorm2d(c, **dict(dict(eps=1e-3, momentum=0.03, step_mode='m'), **kw)).train(train)

    bn = make()
    st = ops.bn_state(bn)
    assert st._fields == ('running_mean', 'running_var', 'batch_stats', 'momentum', 'eps', 'replicas')
    want = dict(train=(bn.running_mean, bn.running_var, True, 0.03, 1),            # batch statistics, running buffers updated
                eval=(bn.running_mean, bn.running_var, False, None, 0),            # running statistics read
                no_running_stats=(None, None, True, None, 0),
                eval_momentum_none=(bn.running_mean, bn.running_var, False, None, 0))[mode]
    assert (st.running_mean is want[0] and st.running_var is want[1] and st.batch_stats is want[2] and st.momentum == want[3]
            and st.eps == 1e-3 and st.replicas == 1)
    if mode != 'no_running_stats':
        assert st.running_mean is not None and int(bn.num_batches_tracked) == want[4]
        ops.bn_state(bn)
        assert int(bn.num_batches_tracked) == 2 * want[4]                          # once per call, never in eval
    with ops.replicated(3):
        assert ops.bn_state(bn).replicas == 3 and ops.bn_state(bn, replicas=1).replicas == 1

    # fused_with and fused_pair hand the kernels exactly this state (one counter bump per layer call)
    seen = []

    def multistep(y, gamma, beta, running_mean, running_var, batch_stats, momentum, eps, *rest, **kwargs):
        seen.append((running_mean, running_var, batch_stats, momentum, eps))
        return torch.zeros_like(y), None, None

    def pair(y12, a, b):
        seen.extend(tuple(lay[3].state[:5]) for lay in (a, b))
        assert a[3].state.replicas == 1 and b[3].state.replicas == 1
        return torch.zeros(1), None, torch.zeros(1), None

    monkeypatch.setattr(ops, 'bn_lif_multistep', multistep)
    monkeypatch.setattr(ops, 'bn_lif_pair', pair)
    bns = [make(), make(), make()]
    nodes = [neuron.LIFNode(surrogate_function=surrogate.ATan(2.0), step_mode='m') for _ in bns]
    bns[0].fused_with(nodes[0], torch.zeros(2, 2, 8, 4, 6))
    layer.fused_pair(bns[1], nodes[1], bns[2], nodes[2], torch.zeros(2, 2, 16, 4, 6))
    assert len(seen) == 3
    for b, got in zip(bns, seen):
        assert got[0] is (b.running_mean if want[0] is not None else None) and got[1] is (b.running_var if want[1] is not None else None)
        assert got[2:] == (want[2], want[3], 1e-3)
        if b.num_batches_tracked is not None:
            assert int(b.num_batches_tracked) == want[4]


def test_bn_state_refuses_the_cumulative_average_in_training():
    with pytest.raises(_lib.EasHipError):
        ops.bn_state(torch.nn.BatchNorm2d(8, momentum=None).train())
