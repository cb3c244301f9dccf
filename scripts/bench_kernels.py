#!/usr/bin/env python3
"""Micro-benchmarks of the hand-written kernels at the benchmark shapes (HIP-event timing, median of repeats).
Development tool; prints achieved GFLOP/s or GB/s per kernel."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import eas_snn_amd  # noqa
from eas_snn_amd import ops


def timeit_spread(fn, reps=20, warm=3):
    """(median, min, max) ms of ``reps`` runs after ``warm`` warm-up runs (HIP events)"""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def timeit(fn, reps=20, warm=3):
    return timeit_spread(fn, reps, warm)[0]


def smallconv(which):
    dev = torch.device('cuda:0')
    for (N, cin, cout) in ((256, 2, 4), (256, 4, 4), (64, 2, 4), (64, 4, 4)):
        H, W, k = 256, 320, 5
        x = torch.randn(N, cin, H, W, device=dev)
        w = torch.randn(cout, cin, k, k, device=dev) * 0.1
        b = torch.randn(cout, device=dev)
        gy = torch.randn(N, cout, H, W, device=dev)
        flops = 2.0 * N * H * W * cin * cout * k * k
        for name, fn in (('fwd', lambda: ops.smallconv_fwd(x, w, b, relu=True)),
                         ('dgrad', lambda: ops.smallconv_bwd_input(gy, w, x)),
                         ('wgrad', lambda: ops.smallconv_bwd_weight(gy, x, w))):
            if which and name not in which:
                continue
            ms = timeit(fn)
            print(f'smallconv {name:5s} N={N:3d} {cin}->{cout} k{k}: {ms:7.3f} ms  {flops / ms / 1e9:8.1f} TFLOP/s' .replace('TFLOP/s', 'GFLOP/ms')
                  + f'  = {flops / (ms * 1e-3) / 1e12:6.2f} TFLOP/s')


# the depthwise layers a depthwise=True SYOLOX-S of config 2 (256x320 canvas, NI = T * B = 192) would have: (C, H, W, stride)
DWCONV_SHAPES = [(32, 128, 160, 2), (32, 64, 80, 1), (64, 64, 80, 2), (64, 32, 40, 1), (128, 32, 40, 2), (128, 16, 20, 1), (256, 16, 20, 2),
                 (256, 8, 10, 1)]


def dwconv(args):
    """eas_dwconv forward (with the BatchNorm statistics epilogue) / input gradient / weight gradient against the library route
    (EAS_DWCONV=0: dense() of the planes where the input is planes, ATen forward + the separate statistics pass, ATen
    convolution_backward) at the same shapes in the same process.  GB/s = the algorithmic bytes of the NATIVE form over the time:
    planes 2 B + fp32 4 B per element read, 4 B per element written."""
    dev = torch.device('cuda:0')
    NI = int(args[0]) if args else 192
    L = eas_snn_amd.hip_library()
    tot = {}
    print(f'NI={NI}; ms = median (min..max) of 20')
    for (C_, H, W, s) in DWCONV_SHAPES:
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        x = (torch.rand(NI, C_, H, W, device=dev) < 0.3).float()
        sp = ops.to_planes(x)
        w = torch.randn(C_, 1, 3, 3, device=dev) / 3
        gy = torch.randn(NI, C_, Ho, Wo, device=dev)
        nx, ny = x.numel(), gy.numel()
        ws = torch.empty(L.eas_bn_workspace_doubles(C_), dtype=torch.float64, device=dev)

        def stats_pass(y):
            return L.eas_bn_stats_partial(ops.ptr(y), 0, NI, C_, Ho * Wo, ops.ptr(ws), ops.stream())

        def native_fwd(xs):
            with ops.conv_stats_scope(True):
                ops.dwconv_fwd(x, w, None, s, xs)
            ops.clear_conv_stats()

        def lib_fwd(from_planes):
            xd = ops.dense(ops.ghost(x.shape, dev, sp)) if from_planes else x
            y = torch.ops.aten.convolution(xd, w, None, (s, s), (1, 1), (1, 1), False, (0, 0), C_)
            assert stats_pass(y) > 0

        def lib_bwd(mask):
            torch.ops.aten.convolution_backward(gy, x, w, None, (s, s), (1, 1), (1, 1), False, (0, 0), C_, mask)

        rows = [
            ('fwd planes', lambda: native_fwd(sp), lambda: lib_fwd(True), 2 * nx + 4 * ny),
            ('fwd fp32', lambda: native_fwd(None), lambda: lib_fwd(False), 4 * nx + 4 * ny),
            ('dgrad', lambda: ops.dwconv_dgrad(gy, w, x.shape, s), lambda: lib_bwd((True, False, False)), 4 * ny + 4 * nx),
            ('wgrad planes', lambda: ops.dwconv_wgrad(x, gy, s, sp), lambda: lib_bwd((False, True, False)), 2 * nx + 4 * ny),
            ('wgrad fp32', lambda: ops.dwconv_wgrad(x, gy, s, None), lambda: lib_bwd((False, True, False)), 4 * nx + 4 * ny),
        ]
        with torch.no_grad():
            for name, native, lib, nbytes in rows:
                a, b = timeit_spread(native), timeit_spread(lib)
                t = tot.setdefault(name, [0.0, 0.0, 0.0, 0.0])
                t[0] += a[0]; t[1] += b[0]; t[2] += a[2] - a[1]; t[3] += b[2] - b[1]
                print(f'dwconv C={C_:3d} {H:3d}x{W:3d} s{s} {name:12s}: native {a[0]:7.3f} ({a[1]:.3f}..{a[2]:.3f}) ms {nbytes / a[0] / 1e6:7.0f} GB/s'
                      f' | library {b[0]:7.3f} ({b[1]:.3f}..{b[2]:.3f}) ms | x{b[0] / a[0]:.2f}', flush=True)
        del x, sp, gy
    for name, t in tot.items():
        print(f'sum over the shapes {name:12s}: native {t[0]:8.3f} ms (sum of spreads {t[2]:.3f}) | library {t[1]:8.3f} ms (sum of spreads {t[3]:.3f})')
    for form in ('planes', 'fp32'):
        a = tot[f'fwd {form}'][0] + tot['dgrad'][0] + tot[f'wgrad {form}'][0]
        b = tot[f'fwd {form}'][1] + tot['dgrad'][1] + tot[f'wgrad {form}'][1]
        print(f'forward + both gradients, {form} input: native {a:.3f} ms | library {b:.3f} ms | x{b / a:.2f}')


def gen4(args):
    """The 1 Mpx training input at config-4 shape (B = 32, Tm = 4, 360 x 640 -> 384 x 640, nbins 10): ``stacked_hist_frames`` from indices
    into a resident store with the letterbox row and with a scale-0.4 jitter row, against the composition it replaces
    (``stacked_hist_event_sum`` of the gathered batch into a sensor-size canvas -> int32 -> ``counts_letterbox``; the gather of the batch is
    not timed).  The forms alternate inside every round.  GB/s = algorithmic bytes over the time: the named source rows once (u8) and the
    frames once (fp32) for the fused form; for the composition also the fp32 sums written and read, the int32 sums written and read."""
    dev = torch.device('cuda:0')
    B = int(args[0]) if args else 32
    Tm, R, H, W, Hc, Wc, nb = 4, 96, 360, 640, 384, 640, 10
    torch.manual_seed(1)
    store = torch.cat([torch.poisson(torch.full((R // 4, 2 * nb, H, W), 0.03, device=dev)).clamp_(max=255).to(torch.uint8) for _ in range(4)])
    first = torch.randperm(R - Tm)[:B].to(dev)                   # 442 MB of representations: more than the 256 MiB last-level cache
    from eas_snn_amd import data
    letter = torch.tensor([data.letterbox_params(H, W, Hc, Wc)] * B, dtype=torch.int32, device=dev)
    nw, nh = int(.4 * Wc), int(int(.4 * Wc) / (W / H))
    small = torch.tensor([(nw, nh, 100 + 3 * b, 50 + 2 * b, b & 1) for b in range(B)], dtype=torch.int32, device=dev)
    gathered = torch.stack([store[int(f):int(f) + Tm] for f in first.tolist()])

    def composition(par):
        sums = ops.stacked_hist_event_sum(gathered, H, W)
        return ops.counts_letterbox(sums.view(B, Tm, 2, H, W).to(torch.int32), par, Hc, Wc)
    assert torch.equal(composition(letter).view(-1), ops.stacked_hist_frames(store, first, Tm, Hc, Wc, params=letter).view(-1))
    assert torch.equal(composition(small).view(-1), ops.stacked_hist_frames(store, first, Tm, Hc, Wc, params=small).view(-1))
    n_in, n_mid, n_out = B * Tm * 2 * nb * H * W, B * Tm * 2 * H * W, B * Tm * 2 * Hc * Wc
    rows_small = min(2 * nh, H)                                 # source rows two taps per output row can name
    forms = [('fused, letterbox row', lambda: ops.stacked_hist_frames(store, first, Tm, Hc, Wc, params=letter), n_in + 4 * n_out),
             ('fused, params None', lambda: ops.stacked_hist_frames(store, first, Tm, Hc, Wc), n_in + 4 * n_out),
             ('fused, scale 0.4 row', lambda: ops.stacked_hist_frames(store, first, Tm, Hc, Wc, params=small), n_in * rows_small // H + 4 * n_out),
             ('composition, letterbox row', lambda: composition(letter), n_in + 16 * n_mid + 4 * n_out),
             ('composition, scale 0.4 row', lambda: composition(small), n_in + 16 * n_mid + 4 * n_out),
             ('event_sum alone (config 4 today)', lambda: ops.stacked_hist_event_sum(gathered, Hc, Wc), n_in + 4 * n_out)]
    print(f'B={B} Tm={Tm} {H}x{W} -> {Hc}x{Wc}')
    alternate(forms)


def letterbox(args):
    """``counts_letterbox`` at the two shapes the front ends run it at: linear at workload 2b's (Gen1, batch 32, Tm = 4, 240 x 304 -> 640 x 640,
    the deterministic letterbox row) and cubic at N-Caltech101's (scripts/dev_atis.py: batch 64, Tl = 1, Tm = 8, 180 x 240 -> 192 x 256).
    GB/s = the int32 counts once + the fp32 frames once over the time."""
    dev = torch.device('cuda:0')
    from eas_snn_amd import data, workloads
    forms = []
    w = workloads.WORKLOADS['2b']
    for name, interp, B, F, (H, W), (Hc, Wc) in (('linear, workload 2b', 'linear', w['batch'], 2 * w['Tm'], w['sensor'], w['canvas']),
                                                 ('cubic, N-Caltech101', 'cubic', 64, 16, (180, 240), (192, 256))):
        counts = torch.poisson(torch.full((B, F, H, W), 0.6, device=dev)).to(torch.int32)
        par = torch.tensor([data.letterbox_params(H, W, Hc, Wc)] * B, dtype=torch.int32, device=dev)
        forms.append((f'{name} {B}x{F} {H}x{W} -> {Hc}x{Wc}', lambda c=counts, q=par, i=interp, hw=(Hc, Wc): ops.counts_letterbox(c, q, *hw, interp=i),
                      4 * B * F * (H * W + Hc * Wc)))
    alternate(forms)


def alternate(forms):
    """5 rounds, the forms (name, fn, algorithmic bytes) alternating inside every round, 20 timed calls each: the median of the round medians,
    their spread (for a comparison of two libraries in one session: scripts/build_variant.sh, EAS_LIB), min..max over all calls"""
    rounds = [[] for _ in forms]
    for _ in range(5):
        for k, (_, fn, _) in enumerate(forms):
            rounds[k].append(timeit_spread(fn, reps=20, warm=3))
    print('ms = median of 5 rounds of (median of 20) [smallest..largest round median] (min..max over all)')
    for (name, _, nbytes), r in zip(forms, rounds):
        meds = sorted(x[0] for x in r)
        med = meds[len(r) // 2]
        print(f'{name:34s}: {med:7.4f} ms [{meds[0]:.4f}..{meds[-1]:.4f}] ({min(x[1] for x in r):.3f}..{max(x[2] for x in r):.3f})  {nbytes / 1e6:7.1f} MB'
              f'  {nbytes / med / 1e6:7.0f} GB/s', flush=True)


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'smallconv'
    if what == 'smallconv':
        smallconv(sys.argv[2:])
    elif what == 'dwconv':
        dwconv(sys.argv[2:])
    elif what == 'gen4':
        gen4(sys.argv[2:])
    elif what == 'letterbox':
        letterbox(sys.argv[2:])
