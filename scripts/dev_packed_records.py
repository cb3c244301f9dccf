#!/usr/bin/env python3
"""Size and time of the Gen1 window store in packed records (``data.Gen1PackedWindowStore``) against ``data.Gen1WindowStore`` on seeded
synthetic recordings: ``--files`` recordings (default 8) of ``--events`` events (default 4 000 000) with ``--labels`` labels (default 16)
``--period-ms`` apart (default 500) and a window of ``--window-ms`` (default 200, the reference's), ``Tl`` = 1, ``Tm`` = 4, the Gen1
sensor on a 256 x 320 canvas with jittered params.

  build        host clock around the construction from the recordings in host memory, ended by a device synchronise; GB/s of SOURCE
               records (8 bytes each).  The upload comes from pageable host memory.
  bytes held   payload + table of the packed store against the records of the window store; narrow and wide blocks
  pack         ``ops.records_pack`` of the first recording's kept records (measure, scan with its one read, pack), and ``ops.records_unpack``
               of all of them: median of ``--rounds`` calls between device events; the unpacked records are compared with the window
               store's first
  frames       ``frames()`` of ``--batch`` samples (default 64) for both stores on the same seeded samples and params, alternated,
               ``--rounds`` calls each (default 20) between device events after 3 warm-up calls: median, minimum, maximum, ``--runs`` times
               (default 3); the results are compared bit for bit first.  Then the range operators alone on the ranges of those batches
               (``event_histogram_dat_ranges`` against ``event_histogram_packed_ranges``), the same way.

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

from eas_snn_amd import data, ops

ap = argparse.ArgumentParser()
ap.add_argument('--files', type=int, default=8)
ap.add_argument('--events', type=int, default=4_000_000)
ap.add_argument('--labels', type=int, default=16)
ap.add_argument('--period-ms', type=int, default=500)
ap.add_argument('--window-ms', type=int, default=200)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--rounds', type=int, default=20)
ap.add_argument('--runs', type=int, default=3)
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


build(data.Gen1PackedWindowStore)                                           # warm-up: code objects, allocator
stores = {}
for cls in (data.Gen1WindowStore, data.Gen1PackedWindowStore):
    stores[cls.__name__], took = build(cls)
    print(f'build {cls.__name__:22s} {took * 1e3:9.1f} ms   {source_bytes / took / 1e9:6.2f} GB/s of source records')
win, packed = stores['Gen1WindowStore'].trim(), stores['Gen1PackedWindowStore'].trim()
blocks = packed.narrow_blocks + packed.wide_blocks
print(f'bytes held    packed {packed.nbytes()} (payload {packed.used_bytes} + table {packed.nbytes() - packed.used_bytes}) against {win.used_bytes} '
      f'= {packed.nbytes() / win.used_bytes:.4f}   kept / total {win.kept_records} / {win.total_records} = {win.kept_records / win.total_records:.4f}')
print(f'blocks        {packed.narrow_blocks} narrow + {packed.wide_blocks} wide: narrow share {packed.narrow_blocks / max(blocks, 1):.5f}')


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


def line(what, v):
    return f'{what}: median {np.median(v) * 1e3:8.1f} us   min {v.min() * 1e3:8.1f}   max {v.max() * 1e3:8.1f}   ({len(v)} calls)'


# the records come back byte for byte: every recording's kept records, from the packed store's logical indices
offs, logical = win.host['file_offsets'], packed.host['file_offsets']
for f in range(len(offs) - 1):
    n = int(offs[f + 1] - offs[f])
    assert torch.equal(packed.unpacked(int(logical[f]), int(logical[f]) + n), win.records[8 * offs[f]:8 * offs[f + 1]]), 'the records differ'
n0 = int(offs[1] - offs[0])
first = win.records[:8 * n0].clone()
table = torch.empty(((n0 + 63) // 64, 2), dtype=torch.int32, device=dev)
arena = torch.empty(8 * 64 * table.shape[0], dtype=torch.uint8, device=dev)
ms = timed(lambda: ops.records_pack(first, table, arena, 0, *SENSOR), WARM + opt.rounds)[WARM:]
print(line(f'pack          ops.records_pack, {n0} records ({8 * n0 / 1e6:.1f} MB)', ms) + f'   {8 * n0 / np.median(ms) / 1e6:.0f} GB/s of records')
total = 64 * blocks
ms = timed(lambda: packed.unpacked(0, total), WARM + opt.rounds)[WARM:]
print(line(f'unpack        ops.records_unpack, {total} records', ms) + f'   {8 * total / np.median(ms) / 1e6:.0f} GB/s of records written')

# frames() of the same samples from both stores
rs = np.random.RandomState(7)
calls = WARM + opt.rounds
idx = [torch.from_numpy(rs.randint(0, len(win), size=opt.batch).astype(np.int64)).to(dev) for _ in range(calls)]
par = torch.tensor([data.jitter_params(*SENSOR, *CANVAS, jitter=.3, rng=rs) for _ in range(opt.batch)], dtype=torch.int32, device=dev)
assert all(torch.equal(win.frames(i, par, exp), packed.frames(i, par, exp)) for i in idx), 'the two stores disagree'
print(f'frames        batch {opt.batch}: {int(sum((win.sample_ranges[i, 0, 1] - win.sample_ranges[i, 0, 0]).sum() for i in idx)) // calls} records per call')
for run in range(opt.runs):
    times = {'Gen1WindowStore': [], 'Gen1PackedWindowStore': []}
    for k in range(calls):                                                  # alternated: a call of one, then the same call of the other
        for name, s in (('Gen1WindowStore', win), ('Gen1PackedWindowStore', packed)):
            ms = timed(lambda: s.frames(idx[k], par, exp), 1)
            if k >= WARM:
                times[name].append(ms[0])
    med = {k: np.median(v) for k, v in times.items()}
    for name, v in times.items():
        print(line(f'frames run {run} {name:22s}', np.asarray(v)))
    print(f'frames run {run} packed / window = {med["Gen1PackedWindowStore"] / med["Gen1WindowStore"]:.3f}')

# the range operators alone
wr, pr = [win.sample_ranges[i].reshape(-1, 2) for i in idx], [packed.sample_ranges[i].reshape(-1, 2) for i in idx]
for run in range(opt.runs):
    times = {'dat_ranges': [], 'packed_ranges': []}
    for k in range(calls):
        for name, fn in (('dat_ranges', lambda: ops.event_histogram_dat_ranges(win.records, wr[k], exp.Tm, *SENSOR)),
                         ('packed_ranges', lambda: ops.event_histogram_packed_ranges(packed.table, packed.payload, pr[k], exp.Tm, *SENSOR))):
            ms = timed(fn, 1)
            if k >= WARM:
                times[name].append(ms[0])
    med = {k: np.median(v) for k, v in times.items()}
    for name, v in times.items():
        print(line(f'histogram run {run} {name:14s}', np.asarray(v)))
    print(f'histogram run {run} packed / dat = {med["packed_ranges"] / med["dat_ranges"]:.3f}')
