"""Writes tests/golden/cocoeval.npz: inputs of ``ops.coco_eval`` and the ``precision`` / ``recall`` arrays the REFERENCE's own native
evaluation (yolox/layers/cocoeval/cocoeval.{h,cpp} of an EAS-SNN checkout) computes for them.

    python scripts/gen_golden_cocoeval.py --reference /path/to/EAS-SNN [--out tests/golden/cocoeval.npz]

The reference's two files are compiled as they stand into a temporary directory outside this repository (g++, pybind11) and driven the way
yolox/layers/fast_coco_eval_api.py drives them: per (image, category) the detections' IoU rows in stable descending-score order cut at
max(maxDets), pycocotools' default parameters.  IoUs are computed here in float64 in the order of pycocotools' bbIou.  Only the .npz is
written: flat input arrays plus ``precision`` [T,R,K,A,M] and ``recall`` [T,K,A,M] per case.  Ground-truth ids are 0..G-1 (the numbering of
the reference's getcocoGT), detection ids 1..D (loadRes).

Every coordinate is a multiple of 1/4 below 2^16 and every score a multiple of 2^-12, i.e. exact in float32: the fixture stores what the
kernels read."""
import argparse
import importlib
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

IOU_THR = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THR = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DETS = [1, 10, 100]


class Case:
    def __init__(self, num_images, num_classes):
        self.I, self.K = num_images, num_classes
        self.det, self.gt = [], []

    def d(self, img, cls, box, score):
        self.det.append((img, cls, [float(v) for v in box], float(score)))

    def g(self, img, cls, box):
        self.gt.append((img, cls, [float(v) for v in box]))

    def arrays(self):
        det_box = np.array([d[2] for d in self.det], np.float32).reshape(-1, 4)
        det_score = np.array([d[3] for d in self.det], np.float32)
        gt_box = np.array([g[2] for g in self.gt], np.float32).reshape(-1, 4)
        assert all(np.array_equal(det_box[j].astype(np.float64), self.det[j][2]) for j in range(len(self.det))), 'box not exact in float32'
        assert all(float(det_score[j]) == self.det[j][3] for j in range(len(self.det))), 'score not exact in float32'
        assert all(np.array_equal(gt_box[j].astype(np.float64), self.gt[j][2]) for j in range(len(self.gt)))
        return dict(det_img=np.array([d[0] for d in self.det], np.int32), det_cls=np.array([d[1] for d in self.det], np.int32),
                    det_box=det_box, det_score=det_score, gt_img=np.array([g[0] for g in self.gt], np.int32),
                    gt_cls=np.array([g[1] for g in self.gt], np.int32), gt_box=gt_box,
                    num_images=np.int64(self.I), num_classes=np.int64(self.K))


def case_empties():
    """(a) detections without GT, GT without detections, neither; (h) a category with GT and no detection anywhere, one with detections and
    no GT anywhere"""
    c = Case(5, 3)
    c.d(0, 0, [10, 10, 40, 40], .75)
    c.d(0, 0, [60, 20, 30, 50], .5)
    c.g(1, 0, [10, 10, 40, 40])
    c.g(1, 0, [100, 20, 30, 30])
    c.g(1, 1, [5, 5, 60, 60])                # category 1: GT only
    c.g(3, 0, [20, 20, 40, 50])
    c.g(3, 0, [120, 40, 100, 100])
    c.d(3, 0, [22, 20, 40, 50], .875)
    c.d(3, 0, [121, 44, 100, 96], .625)
    c.d(3, 0, [200, 10, 20, 20], .25)
    c.d(0, 2, [10, 10, 20, 20], .5)          # category 2: detections only
    c.d(3, 2, [30, 30, 20, 20], .75)
    c.g(3, 1, [130, 30, 50, 50])
    return c


def case_maxdets():
    """(b) one (image, category) list of 130 detections: the cut at 1 / 10 / 100 and the rank"""
    rng = np.random.RandomState(5)
    c = Case(3, 1)
    gts = [[20 + 60 * k, 30, 40, 40] for k in range(5)]
    for g in gts:
        c.g(0, 0, g)
    scores = rng.permutation(130) + 1          # distinct, not in input order
    for j in range(130):
        g = gts[j % 5]
        jit = rng.randint(-24, 25, 4) / 4.0
        c.d(0, 0, [g[0] + jit[0], g[1] + jit[1], g[2] + jit[2], g[3] + jit[3]], scores[j] / 256.0)
    gts1 = [[10, 10, 30, 60], [80, 15, 50, 50], [160, 40, 100, 120]]
    for g in gts1:
        c.g(1, 0, g)
    for j in range(12):
        g = gts1[j % 3]
        jit = rng.randint(-16, 17, 4) / 4.0
        c.d(1, 0, [g[0] + jit[0], g[1] + jit[1], g[2] + jit[2], g[3] + jit[3]], rng.randint(1, 4096) / 4096.0)
    c.g(2, 0, [50, 50, 20, 20])
    c.d(2, 0, [51, 50, 20, 20], .5)
    return c


def case_ties():
    """(c) equal scores inside one image and across images: the stable order decides"""
    rng = np.random.RandomState(7)
    c = Case(4, 2)
    for i in range(4):
        for k in range(2):
            gts = [[15 + 70 * n, 20 + 10 * k, 40, 44] for n in range(3)]
            for g in gts:
                c.g(i, k, g)
            for j in range(9):
                g = gts[j % 3]
                jit = rng.randint(-20, 21, 4) / 4.0
                c.d(i, k, [g[0] + jit[0], g[1] + jit[1], g[2] + jit[2], g[3] + jit[3]], [.25, .5, .75][rng.randint(3)])
    return c


def case_areas():
    """(d) areas exactly 32^2 and 96^2 (inclusive bounds) and clearly inside each range; (f) a detection whose best GT is ignored for the
    range while a worse non-ignored one exists, and unmatched detections outside the range"""
    c = Case(3, 1)
    sizes = [(16, 16), (32, 32), (50, 50), (96, 96), (120, 120), (64, 16), (128, 72)]       # 64x16 = 32^2, 128x72 = 96^2
    x = 0
    for n, (w, h) in enumerate(sizes):
        c.g(0, 0, [x, 10, w, h])
        c.d(0, 0, [x + 1, 10, w, h], (n + 1) / 16.0)
        c.d(0, 0, [x, 200, w, h], (n + 1) / 32.0)            # unmatched, same areas
        x += w + 10
    # (f): GT1 40x40 is 'medium' (ignored for 'small'), GT2 30x30 inside it is 'small'; the 38x38 detection overlaps GT1 more
    c.g(1, 0, [0, 0, 40, 40])
    c.g(1, 0, [4, 4, 30, 30])
    c.d(1, 0, [0, 0, 38, 38], .75)
    c.d(1, 0, [4, 4, 30, 31], .5)
    c.d(1, 0, [300, 300, 120, 120], .875)                    # unmatched and large
    c.d(1, 0, [300, 100, 8, 8], .125)                        # unmatched and small
    # the mirror: the better GT is 'large', the worse one 'medium'
    c.g(2, 0, [0, 0, 100, 100])
    c.g(2, 0, [10, 10, 80, 80])
    c.d(2, 0, [0, 0, 96, 96], .75)
    c.d(2, 0, [10, 10, 80, 84], .625)
    return c


def case_thresholds():
    """(e) IoU exactly at a threshold; (g) two detections competing for one GT at low thresholds, separated at high ones; (i) the annotation
    with id 0 matched by a detection"""
    c = Case(3, 2)
    c.g(0, 0, [0, 0, 10, 10])                                # annotation id 0
    c.d(0, 0, [0, 0, 10, 5], .75)                            # IoU exactly 0.5
    c.g(0, 0, [100, 0, 10, 10])
    c.d(0, 0, [100, 0, 10, 7.5], .5)                         # IoU exactly 0.75
    c.g(0, 0, [200, 0, 16, 16])
    c.d(0, 0, [200, 0, 16, 12], .625)                        # 0.75 again, other numbers
    c.g(0, 0, [300, 0, 20, 20])
    c.d(0, 0, [300, 0, 20, 12], .375)                        # exactly 0.6
    c.d(0, 0, [300, 0, 20, 20], .25)                         # exactly 1.0, arrives after the 0.6 one
    # (g)
    c.g(1, 0, [100, 100, 40, 40])
    c.g(1, 0, [124, 100, 40, 40])
    c.d(1, 0, [102, 100, 40, 40], .875)
    c.d(1, 0, [112, 100, 40, 40], .75)
    c.d(1, 0, [126, 102, 40, 40], .5)
    c.g(1, 1, [10, 10, 50, 30])
    c.d(1, 1, [10, 10, 50, 30], .5)
    c.d(1, 1, [12, 10, 50, 30], .75)
    c.d(1, 1, [14, 12, 50, 30], .875)
    c.g(2, 1, [10, 10, 64, 64])
    c.d(2, 1, [10, 10, 64, 48], .625)                        # exactly 0.75
    c.d(2, 1, [10, 10, 64, 32], .6875)                       # exactly 0.5
    return c


def case_large():
    """(j) about 3000 detections of one category over 40 images (the accumulate kernel walks several chunks with a carry), a second category
    with a few"""
    rng = np.random.RandomState(11)
    c = Case(40, 2)
    for i in range(40):
        gts = []
        for n in range(rng.randint(2, 7)):
            w, h = rng.randint(8, 130), rng.randint(8, 130)
            gts.append([rng.randint(0, 300 - w), rng.randint(0, 240 - h), w, h])
            c.g(i, 0, gts[-1])
        for j in range(rng.randint(60, 90)):
            if rng.rand() < 0.7:
                g = gts[rng.randint(len(gts))]
                s = rng.choice([2, 8, 40])
                jit = rng.randint(-s, s + 1, 4) / 4.0
                box = [g[0] + jit[0], g[1] + jit[1], max(g[2] + jit[2], 1), max(g[3] + jit[3], 1)]
            else:
                w, h = rng.randint(4, 140), rng.randint(4, 140)
                box = [rng.randint(0, 300), rng.randint(0, 240), w, h]
            c.d(i, 0, box, rng.randint(1, 1024) / 1024.0)
        if i % 5 == 0:
            c.g(i, 1, [40, 40, 60, 60])
            c.d(i, 1, [40 + i / 4.0, 40, 60, 60], (i + 1) / 64.0)
    return c


CASES = {'empties': case_empties, 'maxdets': case_maxdets, 'ties': case_ties, 'areas': case_areas, 'thresholds': case_thresholds,
         'large': case_large}


def bb_iou(d, g):
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    return float(i / (d[2] * d[3] + g[2] * g[3] - i))


def build_reference(reference_root, workdir):
    src = os.path.join(reference_root, 'yolox', 'layers', 'cocoeval', 'cocoeval.cpp')
    name = 'eas_ref_cocoeval'
    inc = subprocess.run([sys.executable, '-m', 'pybind11', '--includes'], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    subprocess.run(['g++', '-shared', '-fPIC', '-O2', '-std=c++17', f'-DTORCH_EXTENSION_NAME={name}', *inc, src, '-o',
                    os.path.join(workdir, name + '.so')], check=True)
    sys.path.insert(0, workdir)
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


def run_reference(mod, a):
    I, K = int(a['num_images']), int(a['num_classes'])
    det_box, gt_box = a['det_box'].astype(np.float64), a['gt_box'].astype(np.float64)
    dts = [[[] for _ in range(K)] for _ in range(I)]
    gts = [[[] for _ in range(K)] for _ in range(I)]
    for j in range(len(det_box)):
        dts[a['det_img'][j]][a['det_cls'][j]].append(j)
    for j in range(len(gt_box)):
        gts[a['gt_img'][j]][a['gt_cls'][j]].append(j)
    ious, gt_inst, dt_inst = [], [], []
    for i in range(I):
        ious.append([])
        gt_inst.append([])
        dt_inst.append([])
        for k in range(K):
            dj, gj = dts[i][k], gts[i][k]
            order = np.argsort([-float(a['det_score'][j]) for j in dj], kind='mergesort')[:MAX_DETS[-1]] if dj else []
            ious[-1].append([[bb_iou(det_box[dj[o]], gt_box[g]) for g in gj] for o in order] if dj and gj else [])
            gt_inst[-1].append([mod.InstanceAnnotation(int(g), 0.0, float(gt_box[g][2] * gt_box[g][3]), False, False) for g in gj])
            dt_inst[-1].append([mod.InstanceAnnotation(int(j) + 1, float(a['det_score'][j]), float(det_box[j][2] * det_box[j][3]), False, False)
                                for j in dj])
    area = [[float(v) for v in r] for r in AREA_RNG]
    thr = [float(v) for v in IOU_THR]
    evals = mod.COCOevalEvaluateImages(area, MAX_DETS[-1], thr, ious, gt_inst, dt_inst)
    params = types.SimpleNamespace(recThrs=[float(v) for v in REC_THR], maxDets=list(MAX_DETS), iouThrs=thr, useCats=1, catIds=list(range(K)),
                                   areaRng=area, imgIds=list(range(I)))
    res = mod.COCOevalAccumulate(params, evals)
    counts = list(res['counts'])
    return (np.array(res['precision'], np.float64).reshape(counts), np.array(res['recall'], np.float64).reshape(counts[:1] + counts[2:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of an EAS-SNN checkout (holds yolox/layers/cocoeval/)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'cocoeval.npz'))
    args = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        mod = build_reference(args.reference, tmp)
        for name, make in CASES.items():
            a = make().arrays()
            precision, recall = run_reference(mod, a)
            for k, v in a.items():
                out[f'{name}/{k}'] = v
            out[f'{name}/precision'], out[f'{name}/recall'] = precision, recall
            print(f'{name}: D={len(a["det_score"])} G={len(a["gt_box"])} I={int(a["num_images"])} K={int(a["num_classes"])} '
                  f'AP={precision[precision > -1].mean():.4f} valid={int((precision > -1).sum())}')
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
