#!/usr/bin/env python3
"""Time the N-Caltech101 front end at its README size: 64 synthetic ATIS recordings of 150 000 events, sensor 180x240, Tl=1, Tm=8,
canvas 192x256.  Median of 7 calls after 2 warm-up calls, each call between two device events:

  atis fused        ops.event_histogram_atis on the raw 5-byte records (zero-fill + overflow count + scan + plan + histogram)
  cubic letterbox   ops.counts_letterbox(..., interp='cubic') on its counts
  yardstick         ops.event_histogram on the SAME events decoded on the host (9 B/event struct of arrays), EAS_HIST_FORM=scatter;
                    the band form as well, for information
  host decode       the numpy decode of the batch the fused call makes unnecessary, single-threaded

Development tool.  ``--loop N`` only runs the fused call and the letterbox N times: for a per-kernel split run it under
``rocprofv3 --kernel-trace --stats -- python scripts/dev_atis.py --loop 9`` and read the atis_* rows of kernel_stats.csv."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import eas_snn_amd
from eas_snn_amd import data, ops

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--events', type=int, default=150_000)
ap.add_argument('--loop', type=int, default=0)
opt = ap.parse_args()

H, W, Hc, Wc, Tl, Tm = 180, 240, 192, 256, 1, 8
dev = torch.device('cuda:0')
eas_snn_amd.hip_library()
buf, off = data.synth_atis_batch(opt.batch, opt.events, H, W)
nrec = len(buf) // 5


def host_decode():
    raw = buf.reshape(-1, 5).astype(np.uint32)
    y = raw[:, 1]
    ov = (y == data.ATIS_OVERFLOW_Y)
    c = np.cumsum(ov)
    base = np.concatenate([[0], c])[off[:-1]]                      # overflow records in front of every recording
    t = (((raw[:, 2] & 127) << 16) | (raw[:, 3] << 8) | raw[:, 4]) + data.ATIS_TIME_INCREMENT * (c - np.repeat(base, np.diff(off))).astype(np.uint32)
    ev = ~ov
    n_ev = np.concatenate([[0], np.cumsum(ev)])[off]
    return dict(t=t[ev], x=raw[ev, 0].astype(np.uint16), y=y[ev].astype(np.uint16), p=(raw[ev, 2] >> 7).astype(np.uint8), offsets=n_ev.astype(np.int64))


def median_us(fn, n=7, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


rec, off_dev = torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev)
par = torch.from_numpy(np.array([data.letterbox_params(H, W, Hc, Wc)] * opt.batch, np.int32)).to(dev)
counts = ops.event_histogram_atis(rec, off_dev, Tl, Tm, H, W)
if opt.loop:
    for _ in range(opt.loop):
        ops.counts_letterbox(ops.event_histogram_atis(rec, off_dev, Tl, Tm, H, W), par, Hc, Wc, interp='cubic')
    torch.cuda.synchronize()
    sys.exit(0)

host = []
for _ in range(3):
    t0 = time.perf_counter()
    ev = host_decode()
    host.append((time.perf_counter() - t0) * 1e3)
ev_dev = data.events_to_device(ev, dev)
frames_bytes = 4 * opt.batch * Tl * Tm * 2 * H * W
print(f'{opt.batch} recordings, {nrec} records ({nrec - len(ev["t"])} overflow), {int(counts.sum())} events binned')
rows = [('atis fused', lambda: ops.event_histogram_atis(rec, off_dev, Tl, Tm, H, W), 5 * nrec + frames_bytes),
        ('cubic letterbox', lambda: ops.counts_letterbox(counts, par, Hc, Wc, interp='cubic'), 4 * opt.batch * Tl * Tm * 2 * Hc * Wc)]
for form in ('scatter', 'banded'):
    rows.append((f'event_histogram {form}', lambda: ops.event_histogram(ev_dev['t'], ev_dev['x'], ev_dev['y'], ev_dev['p'], ev_dev['offsets'], Tm, H, W),
                 9 * len(ev['t']) + frames_bytes))
for name, fn, alg in rows:
    if name.startswith('event_histogram'):
        os.environ['EAS_HIST_FORM'] = name.split()[1]
    med, lo, hi = median_us(fn)
    print(f'{name:26s} median {med:9.1f} us  (min {lo:9.1f}, max {hi:9.1f})  {alg / med / 1e3:8.1f} GB/s algorithmic ({alg / 1e6:.0f} MB)', flush=True)
os.environ.pop('EAS_HIST_FORM', None)
print(f'host numpy decode of the batch, single thread: median {np.median(host):.1f} ms of 3')
