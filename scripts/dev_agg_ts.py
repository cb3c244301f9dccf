#!/usr/bin/env python3
"""Time the N-Caltech101 entries of ONE library build, raw through ctypes on buffers allocated once: 32 synthetic ATIS recordings of
200 000 events, sensor 180x240, Tl=1, Tm=8.  Entry after entry, each 3 warm-up calls and then ``--rounds`` (default 20) calls between two
device events; median, minimum and maximum are printed.

  count                    eas_event_histogram_atis               (int32 frames)
  timesurface measure      eas_event_timesurface_atis             (float64 frames: fp64 tanh per event, 64-bit atomic adds, finishing pass)
  latest surface           eas_event_latest_surface_atis          (float64 frames: 64-bit atomic max, in-place exp pass; aggregation 'timesurface')
  latest surface, .dat     eas_event_latest_surface_dat_ranges    (the same events as 8-byte .dat records, one range per recording)

``--lib`` names the build (default: this tree's); a build that lacks the last two entries (the parent commit's) is timed on the first two.
Run it once per build, each in a process of its own with the same order of calls, to see whether the shared kernels kept their speed.
Development tool."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from eas_snn_amd import _lib, data

ap = argparse.ArgumentParser()
ap.add_argument('--lib', default=_lib.LIB_PATH)
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--events', type=int, default=200_000)
ap.add_argument('--rounds', type=int, default=20)
opt = ap.parse_args()

H, W, Tl, Tm = 180, 240, 1, 8
dev = torch.device('cuda:0')
_lib._bind_host_hip_runtime()
lib = ctypes.CDLL(os.path.abspath(opt.lib))
for name, (res, args) in _lib.PROTOTYPES.items():
    if hasattr(lib, name):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args

buf, off = data.synth_atis_batch(opt.batch, opt.events, H, W)
nrec, B = len(buf) // 5, opt.batch
rec, off_dev = torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev)
nbins = B * Tl * Tm * 2 * H * W
counts = torch.empty(nbins, dtype=torch.int32, device=dev)
frames = torch.empty(nbins, dtype=torch.float64, device=dev)
ws = torch.empty(lib.eas_event_timesurface_atis_workspace_bytes(nrec, B, Tl), dtype=torch.uint8, device=dev)
st = _lib.stream


def ok(status):
    assert status == 0, status


rows = [('count', lambda: ok(lib.eas_event_histogram_atis(rec.data_ptr(), nrec, off_dev.data_ptr(), B, 0, 0, Tl, Tm, H, W, counts.data_ptr(), None, None,
                                                          ws.data_ptr(), st())), 10 * nrec + 4 * nbins),
        ('timesurface measure', lambda: ok(lib.eas_event_timesurface_atis(rec.data_ptr(), nrec, off_dev.data_ptr(), B, 0, 0, Tl, Tm, H, W, 500e3,
                                                                          frames.data_ptr(), None, None, ws.data_ptr(), st())), 10 * nrec + 24 * nbins)]
if hasattr(lib, 'eas_event_latest_surface_atis'):
    rows.append(('latest surface', lambda: ok(lib.eas_event_latest_surface_atis(rec.data_ptr(), nrec, off_dev.data_ptr(), B, 0, 0, Tl, Tm, H, W, 10e3,
                                                                                frames.data_ptr(), None, None, ws.data_ptr(), st())), 10 * nrec + 24 * nbins))
    # the same events as .dat records (overflow records dropped), one range per recording
    parts, bounds = [], [0]
    for b in range(B):
        raw = buf[5 * off[b]:5 * off[b + 1]].reshape(-1, 5).astype(np.int64)
        ev = raw[:, 1] != data.ATIS_OVERFLOW_Y
        t = ((((raw[:, 2] & 127) << 16) | (raw[:, 3] << 8) | raw[:, 4]) + data.ATIS_TIME_INCREMENT * np.cumsum(~ev))[ev]
        x, y, p = raw[ev, 0], raw[ev, 1], raw[ev, 2] >> 7
        r = np.empty((len(t), 2), dtype='<u4')
        r[:, 0], r[:, 1] = t, x.astype(np.uint32) | (y.astype(np.uint32) << 14) | (p.astype(np.uint32) << 28)
        parts.append(r)
        bounds.append(bounds[-1] + len(t))
    dat = torch.from_numpy(np.concatenate(parts).view(np.uint8).reshape(-1)).to(dev)
    ranges = torch.tensor([[bounds[b], bounds[b + 1]] for b in range(B)], dtype=torch.int64, device=dev)
    rows.append(('latest surface, .dat', lambda: ok(lib.eas_event_latest_surface_dat_ranges(dat.data_ptr(), ranges.data_ptr(), B, Tm, H, W, 50e3,
                                                                                            frames.data_ptr(), None, st())), 8 * bounds[-1] + 24 * nbins))

print(f'{os.path.abspath(opt.lib)}: {B} recordings, {nrec} records, {opt.rounds} calls after 3 warm-ups', flush=True)
for name, fn, alg in rows:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(opt.rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        t.append(s.elapsed_time(e) * 1e3)
    t = np.asarray(t)
    print(f'{name:22s} median {np.median(t):9.1f} us  (min {t.min():9.1f}, max {t.max():9.1f})  {alg / np.median(t) / 1e3:8.1f} GB/s of '
          f'{alg / 1e6:.0f} MB moved', flush=True)
