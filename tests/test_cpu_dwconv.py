"""CPU-only tests of the depthwise 3x3 convolution route: the C ABI lists the eas_dwconv_* entry points, the static eligibility logic
(``ops.dwconv_form_ok``) has the truth table the kernels are written for, the dense route's own rule is untouched, and a CPU tensor still
gets the module's own result."""
import os
import re

import torch
import torch.nn as nn
import torch.nn.functional as F

import eas_snn_amd
from eas_snn_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DWCONV_ABI = ['eas_dwconv_supported', 'eas_dwconv_fwd_stats_blocks', 'eas_dwconv_fwd', 'eas_dwconv_fwd_planes', 'eas_dwconv_dgrad',
              'eas_dwconv_wgrad_workspace_floats', 'eas_dwconv_wgrad', 'eas_dwconv_wgrad_planes']


class _SubConv(nn.Conv2d):
    pass


def _convs():
    """(module, dwconv_form_ok, _conv_form_ok as before this route existed)"""
    return [
        (nn.Conv2d(16, 16, 3, 1, 1, groups=16), True, False),
        (nn.Conv2d(16, 16, 3, 2, 1, groups=16), True, False),
        (nn.Conv2d(16, 16, 3, 1, 1, groups=2), False, False),
        (nn.Conv2d(8, 16, 3, 1, 1, groups=8), False, False),                 # channel multiplier 2
        (nn.Conv2d(16, 16, 5, 1, 2, groups=16), False, False),
        (nn.Conv2d(16, 16, 3, 1, 2, dilation=2, groups=16), False, False),
        (nn.Conv2d(16, 16, 3, 1, 0, groups=16), False, False),
        (nn.Conv2d(16, 16, 3, 1, 1, groups=16, padding_mode='reflect'), False, False),
        (_SubConv(16, 16, 3, 1, 1, groups=16), False, False),
        (nn.Conv2d(16, 16, 3, 1, 1), False, True),                           # dense: the matrix-core route's, not this one's
        (nn.Conv2d(16, 32, 1, 1, 0), False, True),
    ]


def test_dwconv_entry_points_are_declared_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    for n in DWCONV_ABI:
        assert n in declared, f'{n} is not declared in include/eas_hip.h'
        assert n in eas_snn_amd._lib.PROTOTYPES, f'{n} is not in _lib.PROTOTYPES'
    assert eas_snn_amd._lib.ABI_VERSION == 9                      # purely additive


def test_dwconv_form_truth_table():
    for conv, want_dw, want_dense in _convs():
        assert ops.dwconv_form_ok(conv) is want_dw, conv
        assert bool(ops._conv_form_ok(conv)) is want_dense, conv


def test_switch_is_a_context_field_and_defaults_on():
    assert 'EAS_DWCONV' not in os.environ or os.environ['EAS_DWCONV'] in ('0', '1')
    assert ops.ctx.dwconv is (os.environ.get('EAS_DWCONV', '1') == '1')
    assert ops.DWCONV is ops.ctx.dwconv


def test_cpu_tensor_keeps_the_module_result():
    torch.manual_seed(0)
    conv = nn.Conv2d(16, 16, 3, 2, 1, groups=16)
    x = torch.randn(2, 16, 7, 9)
    assert not ops.dwconv_eligible(x, conv)
    assert torch.equal(ops.conv2d(x, conv), conv(x))


def test_spike_inputs_make_the_fp64_reference_exact_in_fp32():
    """The exactness argument of the GPU tests, confirmed on the CPU: x in {0,1,2} and weights in multiples of 1/8 make every partial sum
    exact in fp32, so torch's fp32 convolution equals the fp64 one bit for bit, whatever the order of its additions."""
    g = torch.Generator().manual_seed(1)
    for C, H, W, s in ((8, 5, 7, 1), (16, 7, 9, 2), (24, 8, 10, 1)):
        x = torch.randint(0, 3, (2, C, H, W), generator=g).float()
        w = torch.randint(-8, 9, (C, 1, 3, 3), generator=g).float() / 8
        y64 = F.conv2d(x.double(), w.double(), None, s, 1, 1, C)
        assert torch.equal(y64.float().double(), y64)
        assert torch.equal(F.conv2d(x, w, None, s, 1, 1, C), y64.float())
