#!/usr/bin/env python3
"""Time the packed-row form of the 1 Mpx store against the u16 form, raw through ctypes on buffers allocated once, at config 4's per-GPU
shape (``workloads.get(4)``: 360x640 sensor, canvas 384x640, batch 32, Tm 4) with jittered params (``jitter_params(..., jitter=.3)``,
seeded), in the procedure of scripts/dev_count_store.py: a store of ``--reps`` representations (default 512: 472 MB as u16), a fresh seeded
draw of indices for every call (the same sequence for both entries), 3 warm-up calls and then ``--rounds`` (default 20) calls between two
device events; median, minimum and maximum are printed.

Three synthetic fillings: Poisson(0.3) per pixel and polarity, with every group of 16 pixels, 40 % and 15 % of the groups kept (the others
zero).  Per filling:

  frames, u16 store        eas_count_store_frames       (indices into uint16 [R, 2, 360, 640])
  frames, packed rows      eas_packed_store_frames      (the same indices into the packed rows of the same sums; the frames must be equal)
  pack, one chunk          eas_count_rows_measure + the scan + eas_count_rows_pack of ``--chunk`` representations (``ops.count_rows_pack``)
  bytes                    u16 store, table + payload of the packed store, and the numpy checker's count (tests/packed_store_ref.py):
                           the last two must agree exactly

Then the build of both stores from host memory (``--build-reps`` representations u8 in two recordings, Poisson(0.03) per bin as
``synth_gen4_recordings`` draws them): ``data.Gen4Store`` and ``data.Gen4PackedStore``, wall time of the second of two builds each.
No figure here says anything about real 1 Mpx recordings: the share of active groups there has not been measured.  Development tool."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import packed_store_ref
from eas_snn_amd import _lib, data, ops, workloads

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=512)
ap.add_argument('--chunk', type=int, default=64)
ap.add_argument('--rounds', type=int, default=20)
ap.add_argument('--build-reps', type=int, default=128)
opt = ap.parse_args()

w = workloads.get(4)
(H, W), (Hc, Wc), B, Tm = w['sensor'], w['canvas'], w['batch'], w['Tm']
R, WARM = opt.reps, 3
dev = torch.device('cuda:0')
lib = _lib.lib()
st = _lib.stream
out = torch.empty((B, 1, Tm, 2, Hc, Wc), dtype=torch.float32, device=dev)
rs = np.random.RandomState(4)
calls = WARM + opt.rounds
first = torch.from_numpy(rs.randint(0, R - Tm + 1, size=(calls, B)).astype(np.int64)).to(dev)
params = torch.tensor([data.jitter_params(H, W, Hc, Wc, jitter=.3, rng=rs) for _ in range(B)], dtype=torch.int32, device=dev)


def ok(status):
    assert status == 0, status


def timed(name, fn, alg=None):
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
    tail = f'  {alg / np.median(t) / 1e3:8.1f} GB/s of {alg / 1e6:.0f} MB moved at most' if alg else ''
    print(f'  {name:22s} median {np.median(t):9.1f} us  (min {t.min():9.1f}, max {t.max():9.1f}){tail}', flush=True)


print(f'sensor {H}x{W}, canvas {Hc}x{Wc}, batch {B}, Tm {Tm}, store of {R} representations, {opt.rounds} calls after {WARM} warm-ups', flush=True)
g = torch.Generator(device=dev).manual_seed(1)
sums = torch.empty((R, 2, H, W), dtype=torch.uint16, device=dev)
rows = torch.empty((R, 2, H, 3), dtype=torch.int64, device=dev)
arena = torch.empty(sums.numel() * 2, dtype=torch.uint8, device=dev)
side = torch.empty_like(arena[:opt.chunk * 2 * H * W * 2])
side_rows = torch.empty_like(rows[:opt.chunk])
n_px, n_out = B * Tm * 2 * H * W, out.numel()
for active in (1.0, 0.4, 0.15):
    for a in range(0, R, 16):
        part = torch.poisson(torch.full((16, 2, H, W), 0.3, device=dev), generator=g)
        keep = (torch.rand((16, 2, H, W // 16), device=dev, generator=g) < active).repeat_interleave(16, dim=3)
        sums.view(torch.int16)[a:a + 16].copy_(part * keep)                     # (sums far below 2^15: the int16 view holds them)
    units = 0
    for a in range(0, R, opt.chunk):                       # chunk by chunk as Gen4PackedStore builds it
        units += ops.count_rows_pack(sums[a:a + opt.chunk], rows[a:a + opt.chunk], arena, units)
    payload = arena[:16 * units]
    want_payload = want_table = 0
    for a in range(0, R, opt.chunk):
        p, t = packed_store_ref.packed_bytes(sums[a:a + opt.chunk].cpu().numpy())
        want_payload, want_table = want_payload + p, want_table + t
    u16, packed = sums.numel() * 2, rows.numel() * 8 + payload.numel()
    print(f'{active:.0%} of the groups active: u16 store {u16} bytes, packed rows {packed} bytes (table {rows.numel() * 8} + payload {payload.numel()}), '
          f'checker {want_table + want_payload} bytes, {u16 / packed:.2f} x smaller', flush=True)
    assert packed == want_table + want_payload, 'the store and the checker count other bytes'

    def frames_u16(i):
        ok(lib.eas_count_store_frames(sums.data_ptr(), R, first[i].data_ptr(), None, params.data_ptr(), B, Tm, H, W, Hc, Wc, out.data_ptr(), None, st()))

    def frames_packed(i):
        ok(lib.eas_packed_store_frames(rows.data_ptr(), payload.data_ptr(), units, R, first[i].data_ptr(), None, params.data_ptr(), B, Tm, H, W, Hc, Wc,
                                       out.data_ptr(), None, st()))

    def pack_chunk(i):
        a = (i * opt.chunk) % (R - opt.chunk + 1)
        ops.count_rows_pack(sums[a:a + opt.chunk], side_rows, side, 0)

    frames_u16(0)
    want = out.clone()
    frames_packed(0)
    assert torch.equal(out, want), 'the packed rows give other frames'
    timed('frames, u16 store', frames_u16, 2 * n_px + 4 * n_out)
    timed('frames, packed rows', frames_packed)
    timed('pack, one chunk', pack_chunk)
del sums, rows, arena, side, side_rows, payload

n = opt.build_reps // 2
block = np.minimum(np.random.default_rng(0).poisson(0.03, size=(16, 20, H, W)), 255).astype(np.uint8)
recs = []
for f, rec in enumerate(data.synth_gen4_recordings(2, 4, (H, W))):
    recs.append((rec[0], np.concatenate([np.roll(block, f + k, axis=0) for k in range((n + 15) // 16)])[:n]) + rec[2:])
print(f'build from host memory: 2 recordings of {n} representations u8 ({2 * n * block[0].nbytes / 1e6:.0f} MB), chunk {opt.chunk}', flush=True)
for cls in (data.Gen4Store, data.Gen4PackedStore, data.Gen4Store, data.Gen4PackedStore):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store = cls(recs, Tm, dev, chunk=opt.chunk)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    size = store.nbytes if cls is data.Gen4PackedStore else store.sums.numel() * 2
    print(f'  {cls.__name__:18s} {dt * 1e3:9.1f} ms, {size} bytes resident', flush=True)
    del store
