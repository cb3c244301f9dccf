#!/usr/bin/env python3
"""Time the two measures of the N-Caltech101 front end on the same records: 32 synthetic ATIS recordings of 200 000 events, sensor 180x240,
Tl=1, Tm=8.  Each call between two device events, after 3 warm-up rounds; the entries alternate inside a round, the median, minimum and
maximum of ``--rounds`` (default 25) rounds are printed:

  count              ops.event_histogram_atis          (int32 frames)
  timesurface        ops.event_timesurface_atis        (float64 frames: fp64 tanh per event, 64-bit atomics, finishing pass)
  count raw, ...     eas_event_histogram_atis of this library and of the one given with --other-lib (e.g. the parent commit's build),
                     both through ctypes on buffers allocated once: says whether the count instance of the shared kernel body kept its speed

Development tool."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import eas_snn_amd
from eas_snn_amd import _lib, data, ops

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--events', type=int, default=200_000)
ap.add_argument('--rounds', type=int, default=25)
ap.add_argument('--other-lib', default=None)
ap.add_argument('--other-first', action='store_true', help='time the other library in front of this one (the call in front of a row decides '
                'what the caches hold: run both orders)')
opt = ap.parse_args()

H, W, Tl, Tm = 180, 240, 1, 8
dev = torch.device('cuda:0')
eas_snn_amd.hip_library()
buf, off = data.synth_atis_batch(opt.batch, opt.events, H, W)
nrec = len(buf) // 5
rec, off_dev = torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev)
nbins = opt.batch * Tl * Tm * 2 * H * W

rows = [('count', lambda: ops.event_histogram_atis(rec, off_dev, Tl, Tm, H, W), 10 * nrec + 4 * nbins),
        ('timesurface', lambda: ops.event_timesurface_atis(rec, off_dev, Tl, Tm, H, W), 10 * nrec + 24 * nbins)]
def raw_count(handle):
    """eas_event_histogram_atis of a library through ctypes on buffers allocated once (the operator allocates frames and workspace per call,
    inside the timed region: the two libraries are compared on this path)"""
    out = torch.empty((opt.batch, Tl, Tm, 2, H, W), dtype=torch.int32, device=dev)
    ws = torch.empty(handle.eas_event_histogram_atis_workspace_bytes(nrec, opt.batch, Tl), dtype=torch.uint8, device=dev)

    def call():
        _lib.check(handle.eas_event_histogram_atis(rec.data_ptr(), nrec, off_dev.data_ptr(), opt.batch, 0, 0, Tl, Tm, H, W, out.data_ptr(), None,
                                                   None, ws.data_ptr(), _lib.stream()), 'eas_event_histogram_atis')
    return call, out


if opt.other_lib:
    other = ctypes.CDLL(os.path.abspath(opt.other_lib))
    for name in ('eas_event_histogram_atis_workspace_bytes', 'eas_event_histogram_atis'):
        getattr(other, name).restype, getattr(other, name).argtypes = _lib.PROTOTYPES[name]
    pair = (('count raw, this lib', _lib.lib()), ('count raw, other lib', other))
    for label, handle in (pair[::-1] if opt.other_first else pair):
        call, out = raw_count(handle)
        call()
        assert torch.equal(out, ops.event_histogram_atis(rec, off_dev, Tl, Tm, H, W)), 'the two libraries count differently'
        rows.append((label, call, 10 * nrec + 4 * nbins))

for _ in range(3):
    for _, fn, _ in rows:
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _, _ in rows}
for _ in range(opt.rounds):
    for name, fn, _ in rows:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times[name].append(s.elapsed_time(e) * 1e3)
frames = ops.event_timesurface_atis(rec, off_dev, Tl, Tm, H, W)
counts = ops.event_histogram_atis(rec, off_dev, Tl, Tm, H, W)
print(f'{opt.batch} recordings, {nrec} records, {int(counts.sum())} events binned, weight sum {float(frames.sum()):.3f}, {opt.rounds} rounds')
for name, _, alg in rows:
    t = np.asarray(times[name])
    print(f'{name:22s} median {np.median(t):9.1f} us  (min {t.min():9.1f}, max {t.max():9.1f})  {alg / np.median(t) / 1e3:8.1f} GB/s of '
          f'{alg / 1e6:.0f} MB moved', flush=True)
