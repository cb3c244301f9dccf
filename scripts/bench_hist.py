#!/usr/bin/env python3
"""Time K1 at the BASELINE size: 64 samples x 200k events, Tm=4, 240x304 -- every form (scatter, banded = 16-bit counters, banded32) of
eas_event_histogram (int32 counts) and of eas_event_frames (fp32 frames on the 256x320 canvas: what the training step calls).
Development tool.  ``--rounds N`` repeats the whole table (one line per form, call and round) for same-box A/B runs of two libraries
(EAS_LIB selects the library)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import eas_snn_amd
from eas_snn_amd import data, ops

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=1)
ap.add_argument('--iters', type=int, default=20)
opt = ap.parse_args()

dev = torch.device('cuda:0')
eas_snn_amd.hip_library()
ev = data.events_to_device(data.synth_event_batch(64, 200_000, seed=0), dev)
args = (ev['t'], ev['x'], ev['y'], ev['p'], ev['offsets'], 4, 240, 304)
calls = {'event_histogram': (lambda: ops.event_histogram(*args), 4 * 64 * 4 * 2 * 240 * 304),
         'event_frames': (lambda: ops.event_frames(*args, 256, 320), 4 * 64 * 4 * 2 * 256 * 320)}
ref = {}
for rnd in range(opt.rounds):
    for form in ('scatter', 'banded', 'banded32'):
        os.environ['EAS_HIST_FORM'] = form
        for name, (fn, out_bytes) in calls.items():
            alg = 9 * ev['t'].numel() + out_bytes
            for _ in range(3):
                out = fn()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(opt.iters):
                out = fn()
            e.record()
            torch.cuda.synchronize()
            ms = s.elapsed_time(e) / opt.iters
            agree = ''
            if name not in ref:
                ref[name] = out.clone()
            elif rnd == 0:
                agree = f'  equals scatter: {bool(torch.equal(ref[name], out))}'
            print(f'round {rnd} {form:8s} {name:16s} {ms * 1e3:8.1f} us  {alg / ms / 1e6:8.1f} GB/s algorithmic ({alg / 1e6:.0f} MB){agree}', flush=True)
