#!/usr/bin/env python3
"""Time the 1 Mpx store entries of ONE library build, raw through ctypes on buffers allocated once, at config 4's per-GPU shape
(``workloads.get(4)``: 360x640 sensor, canvas 384x640, batch 32, Tm 4; nbins 10) with jittered params (``jitter_params(..., jitter=.3)``,
seeded).  Entry after entry, each 3 warm-up calls and then ``--rounds`` (default 20) calls between two device events; median, minimum and
maximum are printed.

  frames, u8 store         eas_stacked_hist_frames      (indices into u8 [R, 20, 360, 640]: 10 byte planes per polarity and source row)
  bin sums, one chunk      eas_stacked_hist_bin_sums    (``--chunk`` representations u8 -> uint16 [chunk, 2, 360, 640] at their place in the store)
  frames, summed store     eas_count_store_frames       (the same indices into uint16 [R, 2, 360, 640])

The store holds ``--reps`` representations (default 512: 2.4 GB as u8, 472 MB summed, so neither form of the store fits the last-level
cache) and every call of a row takes its own seeded draw of indices, the same sequence for both frame entries: a call does not find the
rows of the one before it in a cache.  ``--lib`` names the build (default: this tree's); a build that lacks the last two entries (the
parent commit's) is timed on the first.  Run it once per build, each in a process of its own, to see whether the shared band kernel kept
its speed and what the summed store buys.  Development tool."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from eas_snn_amd import _lib, data, workloads

ap = argparse.ArgumentParser()
ap.add_argument('--lib', default=_lib.LIB_PATH)
ap.add_argument('--reps', type=int, default=512)
ap.add_argument('--chunk', type=int, default=64)
ap.add_argument('--rounds', type=int, default=20)
opt = ap.parse_args()

w = workloads.get(4)
(H, W), (Hc, Wc), B, Tm, nbins = w['sensor'], w['canvas'], w['batch'], w['Tm'], 10
R, WARM = opt.reps, 3
dev = torch.device('cuda:0')
_lib._bind_host_hip_runtime()
lib = ctypes.CDLL(os.path.abspath(opt.lib))
for name, (res, args) in _lib.PROTOTYPES.items():
    if hasattr(lib, name):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args

g = torch.Generator(device=dev).manual_seed(1)
store = torch.empty((R, 2 * nbins, H, W), dtype=torch.uint8, device=dev)
for a in range(0, R, 16):                                  # Poisson(0.03) clamped to 255, as workloads config 4 draws its batch
    part = store[a:a + 16]
    part.copy_(torch.poisson(torch.full(part.shape, 0.03, device=dev), generator=g).clamp_(max=255))
sums = torch.zeros((R, 2, H, W), dtype=torch.uint16, device=dev)
out = torch.empty((B, 1, Tm, 2, Hc, Wc), dtype=torch.float32, device=dev)
rs = np.random.RandomState(4)
calls = WARM + opt.rounds
first = torch.from_numpy(rs.randint(0, R - Tm + 1, size=(calls, B)).astype(np.int64)).to(dev)
params = torch.tensor([data.jitter_params(H, W, Hc, Wc, jitter=.3, rng=rs) for _ in range(B)], dtype=torch.int32, device=dev)
st = _lib.stream


def ok(status):
    assert status == 0, status


def frames_u8(i):
    ok(lib.eas_stacked_hist_frames(store.data_ptr(), R, first[i].data_ptr(), None, params.data_ptr(), B, Tm, nbins, H, W, Hc, Wc, out.data_ptr(), None,
                                   st()))


def bin_sums(i):
    a = (i * opt.chunk) % (R - opt.chunk + 1)
    ok(lib.eas_stacked_hist_bin_sums(store[a:a + opt.chunk].data_ptr(), opt.chunk, nbins, H, W, sums[a:a + opt.chunk].data_ptr(), st()))


def frames_sums(i):
    ok(lib.eas_count_store_frames(sums.data_ptr(), R, first[i].data_ptr(), None, params.data_ptr(), B, Tm, H, W, Hc, Wc, out.data_ptr(), None, st()))


n_px, n_out = B * Tm * 2 * H * W, out.numel()
rows = [('frames, u8 store', frames_u8, nbins * n_px + 4 * n_out)]
if hasattr(lib, 'eas_count_store_frames'):
    for a in range(0, R, opt.chunk):                       # the whole store, chunk by chunk as Gen4Store builds it
        n = min(opt.chunk, R - a)
        ok(lib.eas_stacked_hist_bin_sums(store[a:a + n].data_ptr(), n, nbins, H, W, sums[a:a + n].data_ptr(), st()))
    frames_u8(0)
    want = out.clone()
    frames_sums(0)
    assert torch.equal(out, want), 'the summed store gives other frames'
    rows += [('bin sums, one chunk', bin_sums, opt.chunk * 2 * H * W * (nbins + 2)), ('frames, summed store', frames_sums, 2 * n_px + 4 * n_out)]

print(f'{os.path.abspath(opt.lib)}: sensor {H}x{W}, canvas {Hc}x{Wc}, batch {B}, Tm {Tm}, nbins {nbins}, store of {R} representations, '
      f'{opt.rounds} calls after {WARM} warm-ups', flush=True)
for name, fn, alg in rows:
    for i in range(WARM):
        fn(i)
    torch.cuda.synchronize()
    t = []
    for i in range(WARM, calls):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn(i)
        e.record()
        torch.cuda.synchronize()
        t.append(s.elapsed_time(e) * 1e3)
    t = np.asarray(t)
    print(f'{name:22s} median {np.median(t):9.1f} us  (min {t.min():9.1f}, max {t.max():9.1f})  {alg / np.median(t) / 1e3:8.1f} GB/s of '
          f'{alg / 1e6:.0f} MB moved at most', flush=True)
