"""Operator layer, depthwise 3x3 convolutions (eas_dwconv_*, csrc/dwconv.hip): the ``dconv`` half of ``network_blocks.DWConv``, i.e. every
block of the depthwise=True models (YOLOX-nano family) -- forward on spike planes or fp32 with the BatchNorm statistics in the epilogue,
input gradient, deterministic weight gradient.  ``eas_snn_amd.ops`` re-exports everything here (``ops.<name>``).

EAS_DWCONV=0 (``ctx.dwconv``): development / comparison switch, grouped convolutions go to the library (ATen/MIOpen) as they did before
these kernels existed.  Everything that is not this geometry (5x5, channel multipliers, 1 < groups < C, dilation) stays on the library."""
import torch

from . import _lib
from ._ctx import ctx as opctx
from ._lib import ptr, stream
from .ops_core import _call, _dev, _f32c, _verify_tags, dense, is_small_int, planes_of

_SUPPORT = {}
_BLOCKS = {}


def dwconv_form_ok(conv):
    """what the depthwise kernels ask of the convolution itself (static host logic): a plain nn.Conv2d with one 3x3 filter per channel,
    stride 1 or 2, zero padding 1, no dilation"""
    return (type(conv) is torch.nn.Conv2d and conv.groups == conv.in_channels == conv.out_channels and conv.kernel_size == (3, 3)
            and conv.stride in ((1, 1), (2, 2)) and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.padding_mode == 'zeros')


def _dw_supported(NI, C_, H, W, stride, x_form):
    key = (NI, C_, H, W, stride, x_form)
    r = _SUPPORT.get(key)
    if r is None:
        r = _SUPPORT[key] = bool(_lib.lib().eas_dwconv_supported(*key))
    return r


def dwconv_eligible(x, conv):
    """``conv(x)`` runs on the depthwise kernels: the form above, a CUDA fp32 4-D x, a geometry the library has a tile for"""
    if not (dwconv_form_ok(conv) and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.shape[1] == conv.in_channels and conv.weight.is_cuda and conv.weight.dtype == torch.float32):
        return False
    NI, C_, H, W = x.shape
    return _dw_supported(NI, C_, H, W, conv.stride[0], 1)


def _dw_out_size(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def dwconv_fwd(x, w, bias, stride, x_sp=None):
    """y [NI,C,Ho,Wo] of the depthwise 3x3 convolution of x [NI,C,H,W] (x_sp: x is a ghost, these are its spike planes).  Inside
    ``conv_stats_scope`` (and without bias) the epilogue leaves the BatchNorm partial sums in ``opctx.conv_stats_slot``, exactly as
    ``conv_fwd_packed`` does."""
    L = _lib.lib()
    NI, C_, H, W = x.shape
    Ho, Wo = _dw_out_size(H, W, stride)
    y = torch.empty((NI, C_, Ho, Wo), dtype=torch.float32, device=w.device)
    form = 2 if x_sp is not None else 1
    stats, nb = None, 0
    if opctx.want_conv_stats and bias is None:
        key = (NI, C_, H, W, stride, form)
        nb = _BLOCKS.get(key)
        if nb is None:
            nb = _BLOCKS[key] = L.eas_dwconv_fwd_stats_blocks(*key)
        if 0 < nb <= opctx.conv_stats_max_blocks:
            stats = torch.empty(C_ * nb * 2, dtype=torch.float64, device=y.device)
    fl = 2.0 * y.numel() * 9
    if x_sp is not None:
        assert x_sp.dtype == torch.bfloat16 and tuple(x_sp.shape) == (NI, C_ // 8, H * W, 8)
        x_sp = x_sp.contiguous()
        _call('eas_dwconv', 2 * NI * C_ * H * W + 4 * y.numel(), L.eas_dwconv_fwd_planes, ptr(x_sp), ptr(w), ptr(bias), ptr(y), NI, C_, H, W,
              stride, ptr(stats), nb if stats is not None else 0, stream(), flops=fl)
    else:
        _call('eas_dwconv', 4 * (x.numel() + y.numel()), L.eas_dwconv_fwd, ptr(x), ptr(w), ptr(bias), ptr(y), NI, C_, H, W, stride, ptr(stats),
              nb if stats is not None else 0, stream(), flops=fl)
    if stats is not None:
        opctx.conv_stats_slot = (y, nb, stats, y._version)
    return y


def dwconv_dgrad(gy, w, x_shape, stride):
    """grad_x [NI,C,H,W] from grad_y (eas_dwconv_dgrad)"""
    NI, C_, H, W = x_shape
    gx = torch.empty((NI, C_, H, W), dtype=torch.float32, device=gy.device)
    _call('eas_dwconv', 4 * (gx.numel() + gy.numel()), _lib.lib().eas_dwconv_dgrad, ptr(gy), ptr(w), ptr(gx), NI, C_, H, W, stride, stream(),
          flops=2.0 * gy.numel() * 9)
    return gx


def dwconv_wgrad(x, gy, stride, x_sp=None):
    """grad_w [C,1,3,3] (deterministic: fixed-order partials + a fixed-order reduction in double)"""
    L = _lib.lib()
    NI, C_, H, W = x.shape
    nws = L.eas_dwconv_wgrad_workspace_floats(NI, C_, H, W, stride)
    if nws <= 0:
        raise _lib.EasHipError('eas_dwconv_wgrad: unsupported configuration')
    ws = torch.empty(nws, dtype=torch.float32, device=gy.device)
    gw = torch.empty((C_, 1, 3, 3), dtype=torch.float32, device=gy.device)
    fl = 2.0 * gy.numel() * 9
    if x_sp is not None:
        x_sp = x_sp.contiguous()
        _call('eas_dwconv', 2 * NI * C_ * H * W + 4 * gy.numel(), L.eas_dwconv_wgrad_planes, ptr(x_sp), ptr(gy), ptr(ws), ptr(gw), NI, C_, H, W,
              stride, stream(), flops=fl)
    else:
        _call('eas_dwconv', 4 * (x.numel() + gy.numel()), L.eas_dwconv_wgrad, ptr(x), ptr(gy), ptr(ws), ptr(gw), NI, C_, H, W, stride, stream(),
              flops=fl)
    return gw


class _DwConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, x_sp=None):
        """x_sp: x is a ghost (see ``ghost``) and these are its spike planes: forward and weight gradient read them."""
        _dev(x, w, bias)
        w = _f32c(w)
        bias = _f32c(bias)
        if x_sp is None:
            x = _f32c(x)
        y = dwconv_fwd(x, w, bias, stride, x_sp)
        ctx.save_for_backward(x, w, x_sp)
        ctx.cfg = (stride, bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        from .ops_conv import channel_sum
        x, w, x_sp = ctx.saved_tensors
        stride, has_bias = ctx.cfg
        gy = _f32c(gy)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = dwconv_dgrad(gy, w, x.shape, stride)
        if ctx.needs_input_grad[1]:
            gw = dwconv_wgrad(x, gy, stride, x_sp)
        if has_bias and ctx.needs_input_grad[2]:
            gb = channel_sum(gy)
        return gx, gw, gb, None, None


def dwconv2d(x, conv, small_int=None):
    """``conv(x)`` for a depthwise 3x3 nn.Conv2d on the eas_dwconv kernels (caller checked ``dwconv_eligible``): x is read as spike planes
    when it is a ghost tagged small-int (and the channels come in whole 8-groups), else as fp32."""
    if small_int is None:
        small_int = is_small_int(x)
    sp = planes_of(x)
    if sp is not None and not (small_int and _dw_supported(*x.shape, conv.stride[0], 2)):
        x, sp = dense(x), None
    _verify_tags(x, small_int and sp is not None)
    return _DwConvFn.apply(x, conv.weight, conv.bias, conv.stride[0], sp)
