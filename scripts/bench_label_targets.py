"""Time per step of the label side of a training batch, host path against device op, on the same boxes ("Labels on the device").

    python scripts/bench_label_targets.py [--batch 64] [--reps 500] [--out FILE.json]

Host path: ``SyntheticStackedHistLoader.targets`` -- ``transform_boxes`` per sample, centre form, zero padding in numpy -- followed by the
upload of the [B, 50, 5] array and a device synchronise (a host clock around work that ends in a synchronise).  Device op:
``ops.label_targets`` on a box table that holds the same two boxes per label, indices and draws already on the device (the frame kernels
need them there anyway): device events around ``reps`` launches, and a host clock around the same loop ending in a synchronise (launch
overhead included).  Both paths are warmed up first and their results are compared; they must be equal."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eas_snn_amd import data, ops          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=500)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda', torch.cuda.current_device())
    exp = types.SimpleNamespace(Tm=4, input_size=(384, 640), num_classes=2)
    loader = data.SyntheticStackedHistLoader(exp, args.batch, representations=args.batch)
    idx, par = loader.batches(0)[0]
    (H, W), (Hc, Wc) = loader.sensor_hw, exp.input_size

    def host():
        return torch.from_numpy(loader.targets(idx, par)).to(dev)
    boxes = torch.from_numpy(np.concatenate([loader.raw_boxes(k) for k in range(args.batch)])).to(dev)
    group_start = (torch.arange(args.batch + 1, dtype=torch.int64) * 2).to(dev)
    idx_dev, par_dev = torch.from_numpy(idx).to(dev), torch.from_numpy(par).to(dev)

    def device():
        return ops.label_targets(boxes, group_start, idx_dev, par_dev, H, W, Hc, Wc)
    for _ in range(20):
        a, b = host(), device()
    torch.cuda.synchronize()
    assert torch.equal(a, b), 'host path and device op disagree'
    res = dict(batch=args.batch, reps=args.reps, boxes_per_sample=2, equal=True)
    for rnd in range(3):                                   # the two paths in turn, three rounds: the spread is part of the result
        t0 = time.perf_counter()
        for _ in range(args.reps):
            host()
            torch.cuda.synchronize()
        res.setdefault('host_path_us_per_step', []).append(1e6 * (time.perf_counter() - t0) / args.reps)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        for _ in range(args.reps):
            device()
        e.record()
        torch.cuda.synchronize()
        res.setdefault('device_op_host_clock_us_per_step', []).append(1e6 * (time.perf_counter() - t0) / args.reps)
        res.setdefault('device_op_events_us_per_step', []).append(1e3 * s.elapsed_time(e) / args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
