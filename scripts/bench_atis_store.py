"""Time per call of the N-Caltech101 input of a training step, store path or packed path ("N-Caltech101 from recordings in HBM").

    python scripts/bench_atis_store.py store|packed [--batch 64] [--events 100000] [--files-per-sample 52] [--package DIR]

``store``: ``NCaltechStore.frames`` for ``batch`` recordings of ``events`` events on the 180 x 240 sensor, letterboxed to 192 x 256, picked
out of a resident buffer that holds ``files-per-sample`` times those recordings (the index is made once, outside the timed loop, and timed on
its own).  ``packed``: ``data.atis_to_frames`` on a buffer that holds exactly those recordings back to back -- the best a caller of the packed
entries can do, with the host packing it needs left out.  Both bin the same recordings (the checksum printed must agree).  ``--package``: the
checkout whose ``eas_snn_amd`` is measured (default: this one), so that ``packed`` can be run on an earlier commit built elsewhere.
Warm-up, then device events around 7 windows of 50 back-to-back calls."""
import argparse
import os
import sys
import types

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['store', 'packed'])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--events', type=int, default=100_000)
    ap.add_argument('--files-per-sample', type=int, default=52)
    ap.add_argument('--package', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    import eas_snn_amd
    from eas_snn_amd import data, ops
    B, reps = args.batch, args.files_per_sample
    dev = torch.device('cuda', torch.cuda.current_device())
    print(args.mode, 'package', os.path.dirname(eas_snn_amd.__file__), flush=True)
    base, off = data.synth_atis_batch(B, args.events, seed=3)
    lens = np.diff(off)
    exp = types.SimpleNamespace(Tl=1, Tm=3, input_size=(192, 256), img_size=(180, 240), window=None)
    par = torch.tensor([data.letterbox_params(180, 240, 192, 256)] * B, dtype=torch.int32, device=dev)
    if args.mode == 'packed':
        rec, offsets = torch.from_numpy(base).to(dev), torch.from_numpy(off).to(dev)
        fn = lambda: data.atis_to_frames(rec, offsets, exp, par)
    else:
        # the store repeats the recordings: the size of the resident buffer is what matters here, not its content
        store = data.NCaltechStore.__new__(data.NCaltechStore)
        store.Tl, store.window, store.sensor_hw, store.device = 1, None, (180, 240), dev
        store.records = torch.from_numpy(base).to(dev).repeat(reps)
        store.file_offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(np.tile(lens, reps))]).astype(np.int64)).to(dev)
        store.max_file_records = int(lens.max())
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        store.index = ops.atis_store_index(store.records)
        t1.record()
        torch.cuda.synchronize()
        print(f'store: {B * reps} files, {store.records.numel() / 1e6:.1f} MB, index (once) {t0.elapsed_time(t1):.3f} ms', flush=True)
        # one file of every distinct recording, anywhere in the store: the recordings the packed run bins, in its order
        pick = np.arange(B) + B * np.random.default_rng(0).integers(0, reps, B)
        idx = torch.from_numpy(pick.astype(np.int64)).to(dev)
        fn = lambda: store.frames(idx, par, exp)
    out = fn()
    torch.cuda.synchronize()
    print('frames', tuple(out.shape), 'checksum', float(out.double().sum()), 'records in the batch', int(lens.sum()), flush=True)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(7):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(50):
            fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / 50)
    print(f'RESULT {args.mode}: ms per call, 7 windows of 50: ' + ' '.join(f'{t:.4f}' for t in times) + f'  median {np.median(times):.4f}', flush=True)


if __name__ == '__main__':
    main()
