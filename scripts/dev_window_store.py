#!/usr/bin/env python3
"""Time the Gen1 store that keeps only the records its samples read (``data.Gen1WindowStore``) against the full ``data.Gen1Store`` on
seeded synthetic recordings: ``--files`` recordings (default 8) of ``--events`` events (default 4 000 000) with ``--labels`` labels
(default 16) ``--period-ms`` apart (default 500) and a window of ``--window-ms`` (default 200, the reference's), ``Tl`` = 1, ``Tm`` = 4,
the Gen1 sensor on a 256 x 320 canvas with jittered params.

  build        host clock around the construction from the recordings in host memory, ended by a device synchronise: upload, window search,
               union and gather of every recording; GB/s of SOURCE records (8 bytes each).  The upload comes from pageable host memory.
  gather       ``ops.records_gather`` of the first recording's segments (the build's unit of work, with the wrapper's host check), and
               ``eas_records_gather`` alone on the segments of ALL recordings out of the full store, 50 calls back to back between two
               device events: GB/s of records read plus written (at the default size 2 x 96 MB per call, which the 256 MiB last-level
               cache can hold in part from one call to the next: not a pure HBM rate)
  kept/total   records the store keeps over records it was given
  frames       ``frames()`` of ``--batch`` samples (default 64) for both stores on the same seeded samples and params, alternated,
               ``--rounds`` calls each (default 20) between device events after 3 warm-up calls: median, minimum, maximum; the results
               are compared bit for bit first

Development tool; needs the GPU."""
import argparse
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from eas_snn_amd import _lib, data, ops

ap = argparse.ArgumentParser()
ap.add_argument('--files', type=int, default=8)
ap.add_argument('--events', type=int, default=4_000_000)
ap.add_argument('--labels', type=int, default=16)
ap.add_argument('--period-ms', type=int, default=500)
ap.add_argument('--window-ms', type=int, default=200)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--rounds', type=int, default=20)
opt = ap.parse_args()

assert torch.cuda.is_available(), 'this tool measures on the GPU'
dev = torch.device('cuda:0')
SENSOR, CANVAS, WARM = (240, 304), (256, 320), 3
window = (-opt.window_ms * 1000, 0)
exp = types.SimpleNamespace(Tm=4, Tl=1, input_size=CANVAS, window=-opt.window_ms)
recs = data.synth_gen1_recordings(opt.files, opt.labels, opt.events, SENSOR, label_period_us=opt.period_ms * 1000, seed=3)
source_bytes = sum(len(dat) - data.parse_dat_header(dat)[0] for _, dat, _ in recs)
print(f'{opt.files} recordings x {opt.events} events, {opt.labels} labels {opt.period_ms} ms apart, window {opt.window_ms} ms: '
      f'{source_bytes / 1e6:.1f} MB of records')


def build(cls, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store = cls(recs, 1, window, dev, **kw)
    torch.cuda.synchronize()
    return store, time.perf_counter() - t0


build(data.Gen1WindowStore)                                                 # warm-up: code objects, allocator
for cls in (data.Gen1Store, data.Gen1WindowStore):
    store, took = build(cls)
    print(f'build {cls.__name__:16s} {took * 1e3:9.1f} ms   {source_bytes / took / 1e9:6.2f} GB/s of source records')
    if cls is data.Gen1Store:
        full = store
win = store
print(f'kept / total  {win.kept_records} / {win.total_records} = {win.kept_records / win.total_records:.4f}   '
      f'({win.used_bytes / 1e6:.1f} MB against {full.records.numel() / 1e6:.1f} MB)')


def timed(fn, rounds):
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return np.asarray(out)


# the gather alone, on the first recording
area = recs[0][1][data.parse_dat_header(recs[0][1])[0]:]
rec = torch.from_numpy(area).to(dev)
t = torch.from_numpy(np.unique(recs[0][2]['t']).astype(np.int64)).to(dev)
segments, seg_dst, _ = ops.record_ranges_union(ops.event_window_search(rec, t, window, 1))
n_rec = int(seg_dst[-1])
arena = torch.empty(8 * n_rec, dtype=torch.uint8, device=dev)
ms = timed(lambda: ops.records_gather(rec, segments, seg_dst, arena), WARM + opt.rounds)[WARM:]
print(f'gather        {segments.shape[0]} segments, {n_rec} records, ops.records_gather (with its host check and read): median '
      f'{np.median(ms) * 1e3:.1f} us (min {ms.min() * 1e3:.1f}, max {ms.max() * 1e3:.1f})')
# the kernel alone, on the windows of every recording out of the full store
segments, seg_dst, _ = ops.record_ranges_union(ops.event_window_search(full.records, full.group_t, window, 1, full.file_offsets, full.group_file))
n_rec, seg_src, rec = int(seg_dst[-1]), segments[:, 0].contiguous(), full.records
arena = torch.empty(8 * n_rec, dtype=torch.uint8, device=dev)
assert n_rec == win.kept_records
raw, st, BACK = _lib.lib().eas_records_gather, _lib.stream(), 50


def back_to_back():
    for _ in range(BACK):
        _lib.check(raw(_lib.ptr(rec), _lib.ptr(seg_src), _lib.ptr(seg_dst), segments.shape[0], n_rec, _lib.ptr(arena), st), 'eas_records_gather')


ms = timed(back_to_back, WARM + opt.rounds)[WARM:] / BACK
print(f'gather        eas_records_gather alone, {segments.shape[0]} segments, {n_rec} records, {BACK} calls back to back between two events: median {np.median(ms) * 1e3:.2f} us per call '
      f'(min {ms.min() * 1e3:.2f}, max {ms.max() * 1e3:.2f})   {16 * n_rec / np.median(ms) / 1e6:.0f} GB/s read + written')

# frames() of the same samples from both stores
rs = np.random.RandomState(7)
calls = WARM + opt.rounds
idx = [torch.from_numpy(rs.randint(0, len(full), size=opt.batch).astype(np.int64)).to(dev) for _ in range(calls)]
par = torch.tensor([data.jitter_params(*SENSOR, *CANVAS, jitter=.3, rng=rs) for _ in range(opt.batch)], dtype=torch.int32, device=dev)
assert all(torch.equal(full.frames(i, par, exp), win.frames(i, par, exp)) for i in idx[:2]), 'the two stores disagree'
times = {'Gen1Store': [], 'Gen1WindowStore': []}
for k in range(calls):                                                      # alternated: a call of one, then the same call of the other
    for name, s in (('Gen1Store', full), ('Gen1WindowStore', win)):
        ms = timed(lambda: s.frames(idx[k], par, exp), 1)
        if k >= WARM:
            times[name].append(ms[0])
for name, v in times.items():
    v = np.asarray(v)
    print(f'frames {name:16s} batch {opt.batch}: median {np.median(v) * 1e3:8.1f} us   min {v.min() * 1e3:8.1f}   max {v.max() * 1e3:8.1f}   ({len(v)} calls)')
