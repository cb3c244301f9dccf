"""development: what the device COCO evaluation costs.

  stages    ops.coco_eval on a synthetic detection set of Gen1 scale (2 classes, 60 000 images, up to 100 detections per image and class,
            1-4 ground truths per image and class): device-event time of each stage -- keys, the two sorts (torch.sort), match, accumulate
            -- and of the whole call, after warm-up, median of the repetitions; first the same generator at 100 images against the
            checker (tests/cocoeval_ref.py), bit for bit
  evaluate  EventEvaluator.evaluate of config 2 (SYOLOX-S, batch 64) on the synthetic eval loader with ctx.device_ap on and off in turns:
            off is the route of before the kernels (no AP computed), so the difference is the whole cost of the feature; and that cost
            timed directly: the device feed of every batch plus the AP computation at the end, synchronised before and after

    python scripts/dev_cocoeval.py [stages|evaluate|all] [--images N] [--samples N] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import eas_snn_amd  # noqa: E402,F401
from eas_snn_amd import _lib, ops, workloads  # noqa: E402


def synth(num_images, num_classes=2, max_det=100, seed=0):
    """flat arrays: ground truths on a 304x240 sensor, detections jittered around them or random; coordinates in quarter pixels"""
    rng = np.random.RandomState(seed)
    pairs = num_images * num_classes
    n_gt = rng.randint(1, 5, pairs)
    n_det = rng.randint(0, max_det + 1, pairs)
    gt_pair = np.repeat(np.arange(pairs), n_gt)
    G = len(gt_pair)
    wh = rng.randint(8 * 4, 130 * 4, (G, 2)) / 4.0
    xy = rng.randint(0, 170 * 4, (G, 2)) / 4.0
    gt_box = np.concatenate([xy, wh], 1).astype(np.float32)
    det_pair = np.repeat(np.arange(pairs), n_det)
    D = len(det_pair)
    gt_start = np.concatenate([[0], np.cumsum(n_gt)[:-1]])
    pick = gt_start[det_pair] + (rng.randint(0, 1 << 30, D) % n_gt[det_pair])
    jitter = rng.randint(-1, 2, (D, 4)) * rng.choice([2, 8, 40, 160], (D, 1)) / 4.0
    det_box = gt_box[pick] + jitter.astype(np.float32)
    det_box[:, 2:] = np.maximum(det_box[:, 2:], 1.0)
    det_score = (rng.randint(1, 1 << 16, D) / float(1 << 16)).astype(np.float32)
    return dict(det_img=(det_pair // num_classes).astype(np.int32), det_cls=(det_pair % num_classes).astype(np.int32), det_box=det_box,
                det_score=det_score, gt_img=(gt_pair // num_classes).astype(np.int32), gt_cls=(gt_pair % num_classes).astype(np.int32),
                gt_box=gt_box, num_images=num_images, num_classes=num_classes)


KEYS = ('det_img', 'det_cls', 'det_box', 'det_score', 'gt_img', 'gt_cls', 'gt_box')


def stages(num_images, reps=7):
    import cocoeval_ref
    dev = torch.device('cuda:0')
    small = synth(100, seed=1)
    got = ops.coco_eval(*[torch.from_numpy(small[k]).to(dev) for k in KEYS], 100, 2)
    want = cocoeval_ref.evaluate(*[small[k] for k in KEYS], 100, 2)
    same = bool(np.array_equal(got['precision'].cpu().numpy(), want['precision']) and np.array_equal(got['recall'].cpu().numpy(), want['recall']))
    print(f'100 images, {len(small["det_score"])} detections against the checker: {"bit-equal" if same else "DIFFERENT"}')
    assert same

    case = synth(num_images)
    args = [torch.from_numpy(case[k]).to(dev) for k in KEYS]
    D, G = len(case['det_score']), len(case['gt_img'])
    timer_rows, whole = [], []
    for r in range(2 + reps):
        timer = ops.KernelTimer()
        ops.set_timer(timer)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        res = ops.coco_eval(*args, num_images, 2, max_gt=4)
        e.record()
        torch.cuda.synchronize()
        ops.set_timer(None)
        if r >= 2:                                       # two warm-up calls: code objects, the sorts' temporary storage
            whole.append(s.elapsed_time(e))
            timer_rows.append({k: v['ms'] for k, v in timer.summary().items()})
    stats, _ = ops.coco_summarize(res)
    out = dict(images=num_images, detections=D, ground_truths=G, whole_ms=statistics.median(whole), whole_ms_min=min(whole), whole_ms_max=max(whole),
               ap=float(stats[0]), ap50=float(stats[1]))
    for k in timer_rows[0]:
        out[k + '_ms'] = statistics.median(row[k] for row in timer_rows)
    out['sorts_and_glue_ms'] = out['whole_ms'] - sum(v for k, v in out.items() if k.startswith('eas_'))
    out['ns_per_detection'] = out['whole_ms'] * 1e6 / max(D, 1)
    print(json.dumps(out))
    return out


def evaluate(samples, reps=3):
    dev = torch.device('cuda:0')
    w = workloads.get(2)
    exp = workloads.build_exp(w)
    exp.merge(['test_conf', '0.00003'])
    exp.eval_samples, exp.output_dir = samples, '/tmp/eas_dev_cocoeval'
    torch.manual_seed(80)
    model = exp.get_model().to(dev).eval()
    evaluator = exp.get_evaluator(w['batch'] // 2, False)

    def run(on):
        ops.ctx.device_ap = on
        torch.cuda.synchronize()
        t = time.perf_counter()
        ap, ap50, summary = evaluator.evaluate(model, False, False, None, None, exp.test_size)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, ap, summary
    run(True)                                            # records the graphs
    on, off = [], []
    # order off on on off ...: the loop builds ~10^5 Python records per batch, and the interpreter's full garbage collections (the larger
    # part of that time) fall into every other evaluation -- strictly alternating the two modes measures that rhythm, not the feature
    for k in range(4 * reps):
        mode = k % 4 in (1, 2)
        ms, ap_, summary_ = run(mode)
        (on if mode else off).append(ms)
        if mode:
            ap, summary = ap_, summary_
    # the feature's own pieces, timed directly (synchronised before and after) in one more evaluation
    direct = {}

    def wrap(name):
        fn = getattr(evaluator, name)

        def timed(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn(*a, **k)
            torch.cuda.synchronize()
            direct[name] = direct.get(name, 0.0) + (time.perf_counter() - t) * 1e3
            return r
        setattr(evaluator, name, timed)
    wrap('_feed_device_rows')
    wrap('_device_ap')
    run(True)
    n_det = evaluator.last_coco['detections'] if evaluator.last_coco else 0
    out = dict(samples=samples, batch=evaluator.dataloader.batch_size, evaluate_ms_device_ap=statistics.median(on), evaluate_ms_without=statistics.median(off),
               spread_on=[min(on), max(on)], spread_off=[min(off), max(off)], ap=ap, detections=n_det,
               feed_ms=direct.get('_feed_device_rows', 0.0), device_ap_ms=direct.get('_device_ap', 0.0))
    out['difference_of_medians_ms'] = out['evaluate_ms_device_ap'] - out['evaluate_ms_without']
    out['cost_ms'] = out['feed_ms'] + out['device_ap_ms']
    print(summary)
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    ap_ = argparse.ArgumentParser()
    ap_.add_argument('what', nargs='?', default='all', choices=['stages', 'evaluate', 'all'])
    ap_.add_argument('--images', type=int, default=60_000)
    ap_.add_argument('--samples', type=int, default=256)
    ap_.add_argument('--json', default=None)
    a = ap_.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    _lib.lib()
    result = {}
    if a.what in ('stages', 'all'):
        result['stages'] = stages(a.images)
    if a.what in ('evaluate', 'all'):
        result['evaluate'] = evaluate(a.samples)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(result, f, indent=1)
