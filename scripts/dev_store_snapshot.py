#!/usr/bin/env python3
"""What a store snapshot costs against the build it replaces (``_Store.save`` / ``data.load_store``), on seeded synthetic
recordings written to a temporary directory (``--dir``: where; default the system's), for a Gen1 window store, a Gen1 packed window store
and a packed 1 Mpx store.  Gen1: ``--files`` recordings (default 8) of ``--events`` events (default 4 000 000) with ``--labels`` labels
(default 16) 500 ms apart and the reference's 200 ms window; 1 Mpx: ``--streams`` streams (default 4) of ``--reps`` representations
(default 96) of the 360 x 640 sensor, as ``.npy`` files read through ``numpy.load(mmap_mode='r')``.

  build    host clock around ``from_directories`` + ``trim``, ended by a device synchronise; the files were written a moment ago: a warm
           page cache
  save     host clock around ``save`` (digest on the device, copy out through the pinned buffer, write, rename)
  load     host clock around ``load_store``, ended by a device synchronise: read (warm page cache), upload through the two pinned buffers,
           digest, compare; median of ``--rounds`` (default 3).  The loaded store's device tensors are compared with the built one's.
  digest   ``ops.bytes_digest`` of the store's largest device section, and of a buffer of ``--digest-mb`` (default 1024) random bytes:
           median of ``--calls`` (default 20) between device events after 3 warm-up calls, in GB/s of bytes read
  clone    ``clone()`` of the same buffer in the same process, alternated with the digest call by call, in GB/s of bytes read (the clone
           writes as many again: a digest slower than the clone is not bound by memory)

One JSON line at the end.  Development tool; needs the GPU."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from eas_snn_amd import data, ops

ap = argparse.ArgumentParser()
ap.add_argument('--files', type=int, default=8)
ap.add_argument('--events', type=int, default=4_000_000)
ap.add_argument('--labels', type=int, default=16)
ap.add_argument('--streams', type=int, default=4)
ap.add_argument('--reps', type=int, default=96)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--calls', type=int, default=20)
ap.add_argument('--digest-mb', type=int, default=1024)
ap.add_argument('--chunk-mb', type=int, default=256)
ap.add_argument('--dir', default=None)
opt = ap.parse_args()

assert torch.cuda.is_available(), 'this tool measures on the GPU'
dev = torch.device('cuda:0')
WARM, CHUNK = 3, opt.chunk_mb << 20
WINDOW = (-200_000, 0)


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def digest_and_clone(buf):
    """(digest GB/s, clone GB/s of bytes read, digest ms, clone ms), the two alternated call by call"""
    times = {'digest': [], 'clone': []}
    for k in range(WARM + opt.calls):
        for name, fn in (('digest', lambda: ops.bytes_digest(buf)), ('clone', lambda: buf.clone())):
            ms = timed(fn)
            if k >= WARM:
                times[name].append(ms)
    d, c = float(np.median(times['digest'])), float(np.median(times['clone']))
    return dict(bytes=buf.numel(), digest_ms=round(d, 4), clone_ms=round(c, 4), digest_gbs=round(buf.numel() / d / 1e6, 1),
                clone_gbs=round(buf.numel() / c / 1e6, 1))


def measure(name, build, path):
    build()                                                                     # warm-up: code objects, allocator, page cache
    store, t_build = clocked(build)
    _, t_save = clocked(lambda: store.save(path, chunk_bytes=CHUNK))
    loads = []
    for _ in range(opt.rounds):
        loaded, t = clocked(lambda: data.load_store(path, dev, chunk_bytes=CHUNK))
        loads.append(t)
    fields = type(store)._snapshot_fields['device']
    assert all(torch.equal(getattr(store, k), getattr(loaded, k)) for k in fields), 'the loaded store differs'
    big = max((getattr(store, k) for k in fields), key=lambda t: t.numel() * t.element_size())
    out = dict(file_bytes=os.path.getsize(path), build_s=round(t_build, 4), save_s=round(t_save, 4), load_s=round(float(np.median(loads)), 4),
               build_over_load=round(t_build / float(np.median(loads)), 2), largest_section=digest_and_clone(big.reshape(-1).view(torch.uint8)))
    print(name, json.dumps(out))
    return out


with tempfile.TemporaryDirectory(dir=opt.dir) as tmp:
    gen1 = os.path.join(tmp, 'gen1')
    os.makedirs(gen1)
    for rec_name, dat, rows in data.synth_gen1_recordings(opt.files, opt.labels, opt.events, label_period_us=500_000, seed=3):
        dat.tofile(os.path.join(gen1, f'{rec_name}_td.dat'))
        np.save(os.path.join(gen1, f'{rec_name}_bbox.npy'), rows)
    gen4 = os.path.join(tmp, 'gen4')
    for stream, reps, obj2repr, rows, obj2label, times in data.synth_gen4_recordings(opt.streams, opt.reps, seed=3):
        label_dir = os.path.join(gen4, stream, 'labels_v2')
        rep_dir = os.path.join(gen4, stream, 'event_representations_v2', data.GEN4_REP_NAME)
        os.makedirs(label_dir)
        os.makedirs(rep_dir)
        np.savez(os.path.join(label_dir, 'labels.npz'), labels=rows, objframe_idx_2_label_idx=obj2label)
        np.save(os.path.join(label_dir, 'timestamps_us.npy'), times)
        np.save(os.path.join(rep_dir, 'objframe_idx_2_repr_idx.npy'), obj2repr)
        np.save(os.path.join(rep_dir, 'representations.npy'), reps)
    source = dict(gen1_bytes=sum(os.path.getsize(os.path.join(gen1, f)) for f in os.listdir(gen1)),
                  gen4_bytes=opt.streams * opt.reps * 20 * 360 * 640)

    def read_reps(rep_dir):
        return np.load(os.path.join(rep_dir, 'representations.npy'), mmap_mode='r')
    result = dict(source=source, chunk_bytes=CHUNK)
    result['Gen1WindowStore'] = measure('Gen1WindowStore', lambda: data.Gen1WindowStore.from_directories(gen1, 1, WINDOW, dev).trim(),
                                        os.path.join(tmp, 'window.eas'))
    result['Gen1PackedWindowStore'] = measure('Gen1PackedWindowStore', lambda: data.Gen1PackedWindowStore.from_directories(gen1, 1, WINDOW, dev).trim(),
                                              os.path.join(tmp, 'packed_window.eas'))
    result['Gen4PackedStore'] = measure('Gen4PackedStore', lambda: data.Gen4PackedStore.from_directories(gen4, 4, dev, read_representations=read_reps).trim(),
                                        os.path.join(tmp, 'packed_gen4.eas'))
    g = torch.Generator(device=dev).manual_seed(1)
    result['random_buffer'] = digest_and_clone(torch.randint(0, 256, (opt.digest_mb << 20,), dtype=torch.uint8, device=dev, generator=g))
print(json.dumps(result))
