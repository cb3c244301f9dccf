"""Checker of the device COCO bbox evaluation (``ops.coco_eval``): the same algorithm in plain Python floats (doubles), structured like the
reference's yolox/layers/cocoeval/cocoeval.cpp -- evaluate per (image, category, area range) (:59-197), then accumulate per
(category, area range, max-dets entry, IoU threshold) (:221-369) with the suffix-maximum envelope and ``lower_bound`` written out.
Test infrastructure: imported by tests only.

Conventions shared with the operator: boxes are (x, y, w, h) float32 values widened to double, areas ``w * h``, ``iscrowd`` is always 0,
"matched" means the matched ground truth's id is not 0 (annotation ids count from 0 in this project, so a match to the very first
annotation counts as unmatched while that ground truth is still taken), detection ids are all > 0."""
import bisect

import numpy as np

AREA_NAMES = ['all', 'small', 'medium', 'large']


def default_params():
    """pycocotools' Params('bbox'), bit for bit"""
    return dict(iou_thr=np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
                rec_thr=np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
                area_rng=np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64),
                max_dets=[1, 10, 100])


def bb_iou(d, g):
    """pycocotools maskApi.c bbIou without crowd, in its order of operations"""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] + g[2] * g[3] - i
    return i / u


def _evaluate_pair(dets, gts, iou_thr, area_rng, max_det):
    """dets: [(box, score)] in input order, gts: [(box, id)] in input order -> per area range
    (scores [nd], matches [T][nd] ids, det_ignores [T][nd], gt_ignores [ng])"""
    order = sorted(range(len(dets)), key=lambda j: -dets[j][1])[:max_det]          # stable
    dbox = [[float(v) for v in dets[j][0]] for j in order]
    gbox = [[float(v) for v in g[0]] for g in gts]
    ious = [[bb_iou(d, g) for g in gbox] for d in dbox]
    darea = [d[2] * d[3] for d in dbox]
    garea = [g[2] * g[3] for g in gbox]
    out = []
    for lo, hi in area_rng:
        ign = [a < lo or a > hi for a in garea]
        gorder = sorted(range(len(gts)), key=lambda j: int(ign[j]))                  # stable: non-ignored first
        gign = [ign[j] for j in gorder]
        matches = [[0] * len(order) for _ in iou_thr]
        dign = [[False] * len(order) for _ in iou_thr]
        for t, thr in enumerate(iou_thr):
            taken = [False] * len(gorder)
            for d in range(len(order)):
                best, match = min(float(thr), 1 - 1e-10), -1
                for g in range(len(gorder)):
                    if taken[g]:
                        continue
                    if match >= 0 and not gign[match] and gign[g]:
                        break
                    if ious[d][gorder[g]] >= best:
                        best, match = ious[d][gorder[g]], g
                if match >= 0:
                    dign[t][d] = gign[match]
                    matches[t][d] = int(gts[gorder[match]][1])
                    taken[match] = True
                dign[t][d] = dign[t][d] or (matches[t][d] == 0 and (darea[d] < lo or darea[d] > hi))
        out.append(([float(dets[j][1]) for j in order], matches, dign, gign))
    return out


def evaluate(det_img, det_cls, det_box, det_score, gt_img, gt_cls, gt_box, num_images, num_classes, gt_id=None, iou_thr=None, rec_thr=None,
             area_rng=None, max_dets=(1, 10, 100)):
    """-> dict(precision [T,R,K,A,M], recall [T,K,A,M] float64, counts [K,A] int64: the non-ignored ground truths)"""
    p = default_params()
    iou_thr = [float(v) for v in (p['iou_thr'] if iou_thr is None else iou_thr)]
    rec_thr = [float(v) for v in (p['rec_thr'] if rec_thr is None else rec_thr)]
    area_rng = [[float(v) for v in r] for r in (p['area_rng'] if area_rng is None else area_rng)]
    max_dets = [int(v) for v in max_dets]
    I, K, T, R, A, M = int(num_images), int(num_classes), len(iou_thr), len(rec_thr), len(area_rng), len(max_dets)
    det_box, gt_box = np.asarray(det_box, np.float32).reshape(-1, 4), np.asarray(gt_box, np.float32).reshape(-1, 4)
    det_score = np.asarray(det_score, np.float32).reshape(-1)
    gt_id = np.arange(len(gt_box)) if gt_id is None else np.asarray(gt_id)
    dets = {}
    for j, (i, c) in enumerate(zip(np.asarray(det_img).tolist(), np.asarray(det_cls).tolist())):
        dets.setdefault((i, c), []).append((det_box[j], float(det_score[j])))
    gts = {}
    for j, (i, c) in enumerate(zip(np.asarray(gt_img).tolist(), np.asarray(gt_cls).tolist())):
        gts.setdefault((i, c), []).append((gt_box[j], int(gt_id[j])))
    max_det = max(max_dets) if max_dets else 0
    evals = {}
    for key in set(dets) | set(gts):
        evals[key] = _evaluate_pair(dets.get(key, []), gts.get(key, []), iou_thr, area_rng, max_det)

    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    counts = np.zeros((K, A), np.int64)
    for c in range(K):
        for a in range(A):
            per_image = [evals[(i, c)][a] for i in range(I) if (i, c) in evals]
            npig = sum(1 for e in per_image for g in e[3] if not g)
            counts[c, a] = npig
            for m, md in enumerate(max_dets):
                entries = [(e, d) for e in per_image for d in range(min(len(e[0]), md))]
                entries.sort(key=lambda ed: -ed[0][0][ed[1]])                          # stable: image order, then rank
                if npig == 0:
                    continue
                for t in range(T):
                    tp = fp = 0
                    prec, rec = [], []
                    for e, d in entries:
                        match, ignore = e[1][t][d], e[2][t][d]
                        if match > 0 and not ignore:
                            tp += 1
                        if match == 0 and not ignore:
                            fp += 1
                        rec.append(tp / npig)
                        prec.append(tp / (tp + fp) if tp + fp > 0 else 0.0)
                    recall[t, c, a, m] = rec[-1] if rec else 0.0
                    for j in range(len(prec) - 1, 0, -1):
                        if prec[j] > prec[j - 1]:
                            prec[j - 1] = prec[j]
                    for r, thr in enumerate(rec_thr):
                        j = bisect.bisect_left(rec, thr)
                        precision[t, r, c, a, m] = prec[j] if j < len(prec) else 0.0
    return dict(precision=precision, recall=recall, counts=counts)


def summarize(precision, recall, iou_thr=None, max_dets=(1, 10, 100)):
    """the 12 statistics of COCOeval.summarize (pycocotools cocoeval.py _summarizeDets) from the accumulated arrays"""
    iou_thr = default_params()['iou_thr'] if iou_thr is None else np.asarray(iou_thr, np.float64)

    def one(ap, thr, a, m):
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == iou_thr)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return float(np.mean(s[s > -1])) if len(s[s > -1]) else -1.0
    return np.array([one(1, None, 0, 2), one(1, .5, 0, 2), one(1, .75, 0, 2), one(1, None, 1, 2), one(1, None, 2, 2), one(1, None, 3, 2),
                     one(0, None, 0, 0), one(0, None, 0, 1), one(0, None, 0, 2), one(0, None, 1, 2), one(0, None, 2, 2), one(0, None, 3, 2)])
