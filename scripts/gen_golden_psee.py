"""Writes tests/golden/psee.npz: box sets with timestamps, the flat (image, category, box, score) rows the REFERENCE's Prophesee-protocol code
makes of them, and the ``precision`` / ``recall`` arrays and six statistics the reference's native COCO evaluation computes for those rows.

    python scripts/gen_golden_psee.py --reference /path/to/EAS-SNN [--out tests/golden/psee.npz]

From an EAS-SNN checkout, yolox/utils/psee_loader/io/box_filtering.py and metrics/coco_eval.py are loaded by file path as they stand (the
``pycocotools`` names they import are empty stand-ins: no arithmetic lives there, and the one function that would use them is not called) and
run in the order of evaluation.py's ``evaluate_list``: ``filter_boxes`` on both lists with the camera's thresholds, per file
``_match_times`` over ``np.unique`` of the ground-truth timestamps, ``_to_coco_format`` over all windows.  The rows are then evaluated by
yolox/layers/cocoeval/cocoeval.cpp, compiled into a temporary directory as scripts/gen_golden_cocoeval.py does, with pycocotools' default
parameters and the annotation ids 1..G and areas that ``_to_coco_format`` wrote.  Only the .npz is written.

Every coordinate is a multiple of 1/4 below 512 and every score a multiple of 2^-12 (the 'rounding' case holds free float32 widths and
heights on purpose).  What each case has to contain is asserted here."""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_cocoeval import AREA_RNG, IOU_THR, MAX_DETS, REC_THR, bb_iou, build_reference      # noqa: E402

FIELDS = (('t', '<i8'), ('x', '<f4'), ('y', '<f4'), ('w', '<f4'), ('h', '<f4'), ('class_id', '<u4'), ('track_id', '<u4'),
          ('class_confidence', '<f4'))
# the 40-byte box record of the Prophesee files: the fields packed from byte 0, four bytes of padding
BBOX_DTYPE = np.dtype(dict(names=[n for n, _ in FIELDS], formats=[f for _, f in FIELDS],
                           offsets=np.concatenate([[0], np.cumsum([np.dtype(f).itemsize for _, f in FIELDS])[:-1]]).tolist(), itemsize=40))
CLASSES = {'gen1': ('car', 'pedestrian'), 'gen4': ('pedestrian', 'two-wheeler', 'car')}
SKIP_TS, TOL = 500000, 50000


def thresholds(camera, half):
    diag, side = (60, 20) if camera == 'gen4' else (30, 10)
    return (diag // 2, side // 2) if half else (diag, side)


def load_reference(root):
    """the reference's two modules, by path; ``pycocotools`` is satisfied by empty stand-ins"""
    for name in ('pycocotools', 'pycocotools.coco', 'pycocotools.cocoeval'):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['pycocotools.coco'].COCO = type('COCO', (), {})
    sys.modules['pycocotools.cocoeval'].COCOeval = type('COCOeval', (), {})
    mods = []
    for rel in ('io/box_filtering.py', 'metrics/coco_eval.py'):
        path = os.path.join(root, 'yolox', 'utils', 'psee_loader', rel)
        spec = importlib.util.spec_from_file_location('eas_ref_' + os.path.basename(rel)[:-3], path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


class Files:
    """a list of files, each (ground-truth rows, detection rows); a row is (t, x, y, w, h, cls[, score])"""

    def __init__(self, camera, half=False):
        self.camera, self.half, self.files = camera, half, []

    def file(self):
        self.files.append(([], []))
        return len(self.files) - 1

    def g(self, f, t, box, cls):
        self.files[f][0].append((int(t),) + tuple(box) + (int(cls), 1.0))

    def d(self, f, t, box, cls, score):
        self.files[f][1].append((int(t),) + tuple(box) + (int(cls), score))

    def arrays(self, exact=True):
        def one(rows):
            rows = sorted(rows, key=lambda r: r[0])                       # stable: ascending t, insertion order inside one t
            a = np.zeros(len(rows), BBOX_DTYPE)
            for j, r in enumerate(rows):
                a[j] = (r[0], r[1], r[2], r[3], r[4], r[5], 0, r[6])
                if exact:
                    assert all(float(v) * 4 == int(float(v) * 4) and 0 <= v < 512 for v in r[1:5]), r
                    assert float(r[6]) * 4096 == int(float(r[6]) * 4096), r
            return a
        return [one(g) for g, _ in self.files], [one(d) for _, d in self.files]


def jitter(rng, box, s):
    j = rng.randint(-s, s + 1, 4) / 4.0
    return [max(box[0] + j[0], 0), max(box[1] + j[1], 0), max(box[2] + j[2], 0.25), max(box[3] + j[3], 0.25)]


def score(rng):
    return rng.randint(1, 4096) / 4096.0


def case_filters(camera, half):
    """t = 500000 (dropped) / 500001 (kept); w^2 + h^2 exactly diag^2 (kept) and just below; a side exactly min_side (kept) and 0.25 below
    (dropped), for width and height; the all-zero placeholder row; every class of the camera"""
    rng = np.random.RandomState(3 + len(camera) + int(half))
    D, S = thresholds(camera, half)
    K = len(CLASSES[camera])
    c = Files(camera, half)
    f = c.file()
    big = [40, 30, 3 * D, 2 * D]
    for t in (400000, 500000, 500001):
        c.g(f, t, big, 0)
        c.d(f, t, jitter(rng, big, 8), 0, score(rng))
    sizes = [(0.6 * D, 0.8 * D), (0.6 * D - 0.25, 0.8 * D), (0.8 * D, 0.6 * D), (S, 3 * D), (S - 0.25, 3 * D), (3 * D, S), (3 * D, S - 0.25),
             (S, S), (D, D), (2 * D, 2.5 * D)]
    for n, t in enumerate((600000, 700000, 800000)):
        x = 4.0
        for m, (w, h) in enumerate(sizes):
            box = [x, 20 + 8 * n, w, h]
            c.g(f, t, box, (m + n) % K)
            c.d(f, t, jitter(rng, box, 2), (m + n) % K, score(rng))
            c.d(f, t + rng.randint(-40000, 40000), box, (m + n) % K, score(rng))
            x += 36.0
        c.d(f, t, [0, 0, 0, 0], 0, 0.0)                                    # the placeholder of an image without detections
    f = c.file()                                                           # a file that holds only the placeholder and one label
    c.g(f, 900000, [10, 10, 2 * D, 2 * D], K - 1)
    c.d(f, 900000, [0, 0, 0, 0], 0, 0.0)
    return c


def rounding_pairs(n_each=16):
    """float32 (w, h) near w^2 + h^2 = 30^2 where the decision of the float32 expression with separately rounded products and sum differs
    (a) from the decision in real numbers and (b) from a fused multiply-add form; found by search"""
    rng = np.random.RandomState(17)
    w = rng.uniform(10.5, 28.0, 1_000_000).astype(np.float32)
    h = np.sqrt(900.0 - w.astype(np.float64) ** 2).astype(np.float32)
    step = rng.randint(-1, 2, len(w))                                     # one float32 down, none, one up
    h = np.nextafter(h, np.where(step < 0, np.float32(-np.inf), np.where(step > 0, np.float32(np.inf), h)).astype(np.float32))
    ww, hh = w * w, h * h
    keep32 = (ww + hh) >= np.float32(900)
    w64, h64 = w.astype(np.float64), h.astype(np.float64)
    exact = w64 * w64 + h64 * h64                                         # the products are exact in double; the sum is off by < 2^-43
    sure = np.abs(exact - 900.0) > 1e-9
    keep_real = exact >= 900.0
    fma_a = (w64 * w64 + hh.astype(np.float64)).astype(np.float32) >= np.float32(900)        # fma(w, w, h * h)
    fma_b = (h64 * h64 + ww.astype(np.float64)).astype(np.float32) >= np.float32(900)        # fma(h, h, w * w)
    vs_real = np.where(sure & (keep32 != keep_real))[0]
    vs_fma = np.where(sure & ((keep32 != fma_a) | (keep32 != fma_b)))[0]
    print(f'rounding: {len(vs_real)} pairs differ from the real-number decision, {len(vs_fma)} from an fma form, of {len(w)} draws')
    pick = []
    for idx in (vs_real, vs_fma):
        half = [idx[keep32[idx] == want][:n_each // 2].tolist() for want in (True, False)]     # both directions where both exist
        rest = [j for j in idx[:4 * n_each].tolist() if j not in half[0] and j not in half[1]]
        pick += (half[0] + half[1] + rest)[:n_each]
    assert len(pick) == 2 * n_each, 'the search found too few pairs'
    return w[pick], h[pick], int(np.isin(pick, vs_real).sum()), int(np.isin(pick, vs_fma).sum())


def case_rounding():
    c = Files('gen1')
    f = c.file()
    w, h, n_real, n_fma = rounding_pairs()
    assert n_real >= 8 and n_fma >= 8
    for j, (wj, hj) in enumerate(zip(w, h)):
        t = 600000 + 200000 * (j // 4)
        box = [8.0 + 40 * (j % 4), 16.0, wj, hj]
        c.g(f, t, box, j % 2)
        c.d(f, t, box, j % 2, (j + 1) / 64.0)
        c.d(f, t + 1000, [box[0] + 1, box[1], wj, hj], j % 2, (j + 1) / 128.0)
    return c


def case_windows():
    """detections exactly at ts +- tol and one microsecond outside; labelled timestamps 60 ms apart (windows overlap: duplicated detections);
    several ground truths on one timestamp; a timestamp whose ground truths are all filtered away; a file with ground truth and no
    detections, one with detections and no surviving ground truth, one with detections and no ground truth at all, an empty file; equal
    timestamps in two files; timestamps near 5e9 us"""
    rng = np.random.RandomState(23)
    c = Files('gen1')
    boxes = [[20, 30, 40, 36], [90, 40, 30, 50], [150, 60, 64, 40], [230, 20, 36, 90]]

    def stamps(f, base, cls_shift=0):
        for k, b in enumerate(boxes[:3]):
            c.g(f, base, b, (k + cls_shift) % 2)
        for k, b in enumerate(boxes[2:]):
            c.g(f, base + 60000, jitter(rng, b, 8), k % 2)
        for dt_ in (-TOL - 1, -TOL, -1000, 0, 9999, 10000, 20000, 30000, 40000, TOL, TOL + 1, 60000, 60000 + TOL, 60000 + TOL + 1):
            for k, b in enumerate(boxes):
                c.d(f, base + dt_, jitter(rng, b, 6), k % 2, score(rng))
    f0 = c.file()
    stamps(f0, 1_000_000)
    for b in boxes[:2]:                                                    # a timestamp whose ground truths are all too small: no image
        c.g(f0, 1_500_000, [b[0], b[1], 8, 6], 0)
        c.d(f0, 1_500_000, b, 0, score(rng))
        c.d(f0, 1_500_000 + 20000, jitter(rng, b, 4), 1, score(rng))
    c.g(f0, 2_000_000, boxes[3], 1)
    c.d(f0, 2_000_000 - 30000, [boxes[3][0], boxes[3][1], 6, 6], 1, score(rng))       # a detection the filter drops inside a window
    c.d(f0, 2_000_000 + 30000, jitter(rng, boxes[3], 4), 1, score(rng))
    f1 = c.file()                                                          # ground truth, no detections
    c.g(f1, 800_000, boxes[0], 0)
    c.g(f1, 900_000, boxes[1], 1)
    f2 = c.file()                                                          # detections, ground truth that does not survive (too early, too small)
    c.g(f2, 300_000, boxes[0], 0)
    c.g(f2, 700_000, [10, 10, 9.75, 40], 1)
    for t in (300_000, 700_000, 720_000):
        c.d(f2, t, boxes[0], 0, score(rng))
    c.file()                                                               # empty
    f4 = c.file()                                                          # the timestamps of file 0 again: other images
    stamps(f4, 1_000_000, cls_shift=1)
    f5 = c.file()                                                          # detections, no ground truth rows at all
    c.d(f5, 1_000_000, boxes[1], 1, score(rng))
    f6 = c.file()                                                          # beyond 2^32 us
    stamps(f6, 5_000_000_000)
    c.file()                                                               # a trailing empty file
    return c


def case_large():
    """40 files x 20 timestamps, about 3000 detections; file 7 alone holds 2000 of them on timestamps 30 ms apart (more than 1024 kept rows
    in one file, windows of more than 256 rows, every detection in several images)"""
    rng = np.random.RandomState(29)
    c = Files('gen4', True)
    for f in range(40):
        c.file()
        dense = f == 7
        step = 30000 if dense else 150000
        base = 600_000 + 10_000 * f
        all_gts = []
        for s in range(20):
            t = base + s * step
            gts = []
            for n in range(rng.randint(1, 4)):
                w, h = rng.randint(8, 130), rng.randint(8, 130)
                gts.append(([rng.randint(0, 300), rng.randint(0, 240), w, h], rng.randint(3)))
                c.g(f, t, *gts[-1])
            all_gts.append((t, gts))
        n_det = 2000 if dense else 28
        for j in range(n_det):
            t, gts = all_gts[rng.randint(20)]
            g, cls = gts[rng.randint(len(gts))]
            if rng.rand() < 0.7:
                box = jitter(rng, g, rng.choice([2, 8, 40]))
            else:
                box, cls = [rng.randint(0, 300), rng.randint(0, 240), rng.randint(4, 140), rng.randint(4, 140)], rng.randint(3)
            c.d(f, t + rng.randint(-70000, 70001), box, cls, score(rng))
    return c


def case_samples():
    """the evaluator's shape: every sample its own file with one timestamp (sample i at i * 100 ms: the first six fall to the time filter),
    some samples with only the placeholder row"""
    rng = np.random.RandomState(31)
    c = Files('gen1')
    for i in range(64):
        f = c.file()
        t = i * 100_000
        gts = []
        for n in range(rng.randint(1, 4)):
            lo = 30 if n == 0 else 6                                       # the first label of a sample always passes the size filter
            gts.append([rng.randint(0, 200), rng.randint(0, 150), rng.randint(lo, 90), rng.randint(lo, 80)])
            c.g(f, t, gts[-1], rng.randint(2))
        if i % 9 == 4:
            c.d(f, t, [0, 0, 0, 0], 0, 0.0)
            continue
        for j in range(rng.randint(1, 9)):
            c.d(f, t, jitter(rng, gts[rng.randint(len(gts))], rng.choice([2, 12, 60])), rng.randint(2), score(rng))
    return c


CASES = {'filters_gen1': lambda: case_filters('gen1', False), 'filters_gen4': lambda: case_filters('gen4', False),
         'filters_gen4_half': lambda: case_filters('gen4', True), 'rounding': case_rounding, 'windows': case_windows, 'large': case_large,
         'samples': case_samples}


def reference_rows(filt, coco, gts, dts, camera, half):
    """evaluate_list + evaluate_detection of the reference up to the COCO dictionaries, then those as flat arrays"""
    diag, side = thresholds(camera, half)
    gts_f = [filt.filter_boxes(g, SKIP_TS, diag, side) for g in gts]
    dts_f = [filt.filter_boxes(d, SKIP_TS, diag, side) for d in dts]
    flat_gt, flat_dt, image_file, image_t = [], [], [], []
    for f, (g, d) in enumerate(zip(gts_f, dts_f)):
        all_ts = np.unique(g['t'])
        gw, dw = coco._match_times(all_ts, g, d, TOL)
        flat_gt += gw
        flat_dt += dw
        image_file += [f] * len(all_ts)
        image_t += [int(t) for t in all_ts]
    categories = [{'id': k + 1, 'name': n, 'supercategory': 'none'} for k, n in enumerate(CLASSES[camera])]
    dataset, results = coco._to_coco_format(flat_gt, flat_dt, categories, height=240, width=304)
    ann = dataset['annotations']
    rows = dict(gt_img=np.array([a['image_id'] - 1 for a in ann], np.int32), gt_cls=np.array([a['category_id'] - 1 for a in ann], np.int32),
                gt_box=np.array([a['bbox'] for a in ann], np.float32).reshape(-1, 4), gt_id=np.array([a['id'] for a in ann], np.int64),
                det_img=np.array([r['image_id'] - 1 for r in results], np.int32),
                det_cls=np.array([r['category_id'] - 1 for r in results], np.int32),
                det_box=np.array([r['bbox'] for r in results], np.float32).reshape(-1, 4),
                det_score=np.array([r['score'] for r in results], np.float32),
                image_file=np.array(image_file, np.int32), image_t=np.array(image_t, np.int64))
    assert len(dataset['images']) == len(image_t)
    gt_area = [float(a['area']) for a in ann]
    det_area = [float(r['bbox'][2] * r['bbox'][3]) for r in results]      # loadRes: bbox[2] * bbox[3] of the (float32) values it is given
    kept = (sum(len(g) for g in gts_f), sum(len(d) for d in dts_f))
    return rows, gt_area, det_area, kept


def run_native(mod, rows, gt_area, det_area, I, K):
    """COCOevalEvaluateImages + COCOevalAccumulate of the reference's native module over the rows (as gen_golden_cocoeval.run_reference drives
    it), with the annotation ids and areas of _to_coco_format"""
    det_box, gt_box = rows['det_box'].astype(np.float64), rows['gt_box'].astype(np.float64)
    dts = [[[] for _ in range(K)] for _ in range(I)]
    gts = [[[] for _ in range(K)] for _ in range(I)]
    for j in range(len(det_box)):
        dts[rows['det_img'][j]][rows['det_cls'][j]].append(j)
    for j in range(len(gt_box)):
        gts[rows['gt_img'][j]][rows['gt_cls'][j]].append(j)
    ious, gt_inst, dt_inst = [], [], []
    for i in range(I):
        ious.append([])
        gt_inst.append([])
        dt_inst.append([])
        for k in range(K):
            dj, gj = dts[i][k], gts[i][k]
            order = np.argsort([-float(rows['det_score'][j]) for j in dj], kind='mergesort')[:MAX_DETS[-1]] if dj else []
            ious[-1].append([[bb_iou(det_box[dj[o]], gt_box[g]) for g in gj] for o in order] if dj and gj else [])
            gt_inst[-1].append([mod.InstanceAnnotation(int(rows['gt_id'][g]), 0.0, gt_area[g], False, False) for g in gj])
            dt_inst[-1].append([mod.InstanceAnnotation(int(j) + 1, float(rows['det_score'][j]), det_area[j], False, False) for j in dj])
    area = [[float(v) for v in r] for r in AREA_RNG]
    thr = [float(v) for v in IOU_THR]
    evals = mod.COCOevalEvaluateImages(area, MAX_DETS[-1], thr, ious, gt_inst, dt_inst)
    params = types.SimpleNamespace(recThrs=[float(v) for v in REC_THR], maxDets=list(MAX_DETS), iouThrs=thr, useCats=1, catIds=list(range(K)),
                                   areaRng=area, imgIds=list(range(I)))
    res = mod.COCOevalAccumulate(params, evals)
    counts = list(res['counts'])
    return (np.array(res['precision'], np.float64).reshape(counts), np.array(res['recall'], np.float64).reshape(counts[:1] + counts[2:]))


def six_stats(precision):
    """stats[0:6] of COCOeval.summarize: mean over the entries > -1 of AP, AP50, AP75 (all areas), AP small / medium / large, maxDets 100"""
    def one(thr, a):
        s = precision if thr is None else precision[np.where(thr == IOU_THR)[0]]
        s = s[:, :, :, a, 2]
        return float(np.mean(s[s > -1])) if len(s[s > -1]) else -1.0
    return np.array([one(None, 0), one(.5, 0), one(.75, 0), one(None, 1), one(None, 2), one(None, 3)], np.float64)


def check_case(name, c, gts, dts, rows, kept):
    """the case really holds what it is there for"""
    D, S = thresholds(c.camera, c.half)
    all_g, all_d = np.concatenate(gts), np.concatenate(dts)
    if name.startswith('filters'):
        for a in (all_g, all_d):
            assert (a['t'] == 500000).any() and (a['t'] == 500001).any()
            assert ((a['w'] == 0.6 * D) & (a['h'] == 0.8 * D)).any() and ((a['w'] == S) | (a['h'] == S)).any()
            assert ((a['w'] == S - 0.25) | (a['h'] == S - 0.25)).any()
        assert ((all_d['w'] == 0) & (all_d['h'] == 0) & (all_d['class_confidence'] == 0)).any()
        assert 500001 in rows['image_t'] and 500000 not in rows['image_t']
        assert ((rows['gt_box'][:, 2] == 0.6 * D) & (rows['gt_box'][:, 3] == 0.8 * D)).any() and (rows['gt_box'][:, 2:] >= S).all()
        assert len(np.unique(all_g['class_id'])) == len(CLASSES[c.camera])
    if name == 'windows':
        assert len(rows['det_img']) > kept[1], 'no detection is duplicated'
        assert len(np.unique(rows['image_t'])) < len(rows['image_t']) and rows['image_t'].max() > 2 ** 32
        assert 1_500_000 not in rows['image_t']
        per_file = [int((rows['image_file'] == f).sum()) for f in range(len(gts))]
        assert per_file[1] > 0 and per_file[2] == 0 and per_file[3] == 0 and per_file[5] == 0
        assert not np.isin(rows['det_img'], np.where(rows['image_file'] == 1)[0]).any()
        assert np.bincount(rows['gt_img']).max() >= 3
    if name == 'large':
        assert len(gts) == 40 and len(rows['image_t']) >= 700 and len(all_d) >= 3000
        win = np.bincount(rows['det_img'], minlength=len(rows['image_t']))
        assert win.max() > 256 and len(rows['det_img']) > kept[1] and max(len(d) for d in dts) > 1024
        pairs = np.bincount(rows['gt_img'].astype(np.int64) * 3 + rows['gt_cls'])
        assert pairs.max() <= 64
    if name == 'samples':
        assert len(gts) == 64 and all(len(np.unique(g['t'])) == 1 for g in gts) and len(rows['image_t']) == 58


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of an EAS-SNN checkout')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'psee.npz'))
    args = ap.parse_args()
    filt, coco = load_reference(args.reference)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        mod = build_reference(args.reference, tmp)
        for name, make in CASES.items():
            c = make()
            gts, dts = c.arrays(exact=name != 'rounding')
            rows, gt_area, det_area, kept = reference_rows(filt, coco, gts, dts, c.camera, c.half)
            check_case(name, c, gts, dts, rows, kept)
            I, K = len(rows['image_t']), len(CLASSES[c.camera])
            precision, recall = run_native(mod, rows, gt_area, det_area, I, K)

            def field(arrs, k, dtype):
                return np.concatenate([a[k] for a in arrs]).astype(dtype)
            for side, arrs in (('gt', gts), ('dt', dts)):
                out[f'{name}/{side}_t'] = field(arrs, 't', np.int64)
                out[f'{name}/{side}_box'] = np.stack([field(arrs, k, np.float32) for k in 'xywh'], 1)
                out[f'{name}/{side}_cls'] = field(arrs, 'class_id', np.int32)
                out[f'{name}/{side}_offsets'] = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
            out[f'{name}/dt_score'] = field(dts, 'class_confidence', np.float32)
            out[f'{name}/camera'] = np.array(c.camera)
            out[f'{name}/downsampled_by_2'] = np.int64(c.half)
            out[f'{name}/time_tol'] = np.int64(TOL)
            for k, v in rows.items():
                out[f'{name}/out_{k}'] = v
            out[f'{name}/num_images'] = np.int64(I)
            out[f'{name}/kept'] = np.array(kept, np.int64)
            out[f'{name}/precision'], out[f'{name}/recall'], out[f'{name}/stats'] = precision, recall, six_stats(precision)
            print(f'{name}: files={len(gts)} gt={len(out[name + "/gt_t"])} dt={len(out[name + "/dt_t"])} kept={kept} images={I} '
                  f'G={len(rows["gt_img"])} D={len(rows["det_img"])} stats={np.round(six_stats(precision), 4).tolist()}')
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
