"""Writes tests/golden/gen1_labels.npz: synthetic Gen1 boxes and what the REFERENCE's own label path makes of them --
``GEN1Dataset.get_random_data`` (random branch and both deterministic branches), ``reformat('cxcywh')`` and ``TrainTransform.__call__``.

    python scripts/gen_golden_gen1_labels.py --reference /path/to/EAS-SNN [--out tests/golden/gen1_labels.npz]

yolox/data/datasets/gen1.py is loaded by file location under its package name with empty stand-ins for what it imports, except
yolox/utils/boxes.py (loaded for real, ``torchvision`` stubbed) and yolox/data/event_data_augment.py (``TrainTransform``, loaded for real).
``get_random_data`` runs unbound on a namespace whose ``batch_resize`` returns zeros of the asked size and records ``dsize``, whose ``rand``
calls ``np.random.rand`` as the reference's does and records each draw, and whose ``letterbox_image`` is true, then false.  The box rows
carry a sixth column with their row number, so the output tells which rows survived and in which order; the full permutation is
``np.random.shuffle`` of ``arange(n)`` replayed from the same state, and the survivors' order is asserted to agree with it.  No bytecode is
written into the reference tree.  Only data is stored, one array per field over the C cases ``names``: ``sensor`` (ih, iw), ``canvas``
(h, w), ``branch`` (0 random, 1 letterbox, 2 plain resize), ``draws`` float64 [C, 6] (zeros in the deterministic branches, which draw
none), ``dsize`` (nw, nh), ``targets`` float32 [C, 50, 5]; ``raw`` float32 [sum n, 5] (x1, y1, x2, y2, class) and ``perm`` int64 [sum n],
case c at ``raw_offsets[c] .. raw_offsets[c + 1]``; ``boxes`` float32 [sum k, 5] (after get_random_data) and ``rows`` int64 [sum k] (their
row numbers), case c at ``box_offsets[c] .. box_offsets[c + 1]``."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True

GEOMETRIES = {'gen1': ((240, 304), (256, 320)), 'small': ((36, 48), (64, 64))}


class _Stub(types.ModuleType):
    """an empty module: every name it is asked for is a do-nothing class"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        cls = type(name, (), {'mosaic_getitem': staticmethod(lambda fn: fn), 'info': staticmethod(lambda *a, **k: None)})
        setattr(self, name, cls)
        return cls


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(root):
    for name in ('cv2', 'loguru', 'tqdm', 'torchvision', 'yolox', 'yolox.data', 'yolox.data.datasets', 'yolox.data.datasets.datasets_wrapper',
                 'yolox.data.datasets.gen1_classes', 'yolox.utils', 'yolox.utils.util', 'yolox.utils.psee_loader', 'yolox.utils.psee_loader.io',
                 'yolox.utils.psee_loader.io.psee_loader', 'yolox.utils.cache', 'yolox.utils.event_reps'):
        sys.modules[name] = _Stub(name)
    boxes = _load('yolox.utils.boxes', os.path.join(root, 'yolox', 'utils', 'boxes.py'))
    sys.modules['yolox.utils'].xyxy2cxcywh, sys.modules['yolox.utils'].normalize_box = boxes.xyxy2cxcywh, boxes.normalize_box
    dataset = _load('yolox.data.datasets.gen1', os.path.join(root, 'yolox', 'data', 'datasets', 'gen1.py')).GEN1Dataset
    transform = _load('yolox.data.event_data_augment', os.path.join(root, 'yolox', 'data', 'event_data_augment.py')).TrainTransform
    return dataset, transform


def box_sets(ih, iw):
    """name -> rows (x1, y1, x2, y2, class) on an ih x iw sensor"""
    rng = np.random.default_rng(ih * 1000 + iw)
    u = iw / 304.0                                                            # the 'gen1' numbers, shrunk for the small sensor
    many = []
    for k in range(70):                                                       # inside the sensor and large: every one survives every draw
        bw, bh = rng.uniform(0.25, 0.4) * iw, rng.uniform(0.3, 0.45) * ih
        x, y = rng.uniform(0.05 * iw, 0.95 * iw - bw), rng.uniform(0.05 * ih, 0.95 * ih - bh)
        many.append((x, y, x + bw, y + bh, k % 2))
    return {
        'none': np.zeros((0, 5)),
        'one': [(60.3 * u, 50.7 * u, 160.9 * u, 130.2 * u, 1)],
        # negative corners: truncation toward zero is not floor there (-7.6 -> -7)
        'negative': [(-7.6, -3.2, 140.5 * u, 130.9 * u, 1), (-0.5, -0.9, 90.0 * u, 100.0 * u, 0), (-30.7 * u, 20.1 * u, 80.4 * u, 99.9 * u, 1),
                     (50.2 * u, -41.8 * u, 120.6 * u, 60.3 * u, 0)],
        # one box across each border, one across two, one that covers the sensor
        'borders': [(-20 * u, 40 * u, 70 * u, 120 * u, 0), (250 * u, 60 * u, iw + 25 * u, 150 * u, 1), (100 * u, -15 * u, 180 * u, 60 * u, 0),
                    (90 * u, 180 * u, 170 * u, ih + 30 * u, 1), (260 * u, 200 * u, iw + 9, ih + 7, 0), (-5, -5, iw + 5, ih + 5, 1)],
        # at most one pixel wide or high after the scaling, next to boxes that stay
        'tiny': [(100 * u, 100 * u, 100 * u + 1, 160 * u, 0), (40 * u, 70 * u, 120 * u, 70 * u + 1.9, 1), (150.2 * u, 30 * u, 150.9 * u, 90 * u, 0),
                 (200 * u, 100 * u, 200 * u, 100 * u, 1), (30 * u, 20 * u, 110 * u, 95 * u, 1), (10.5 * u, 120.5 * u, 12.4 * u, 122.4 * u, 0)],
        'many': many,
    }


def run_case(Dataset, Transform, raw, sensor, canvas, branch, seed):
    """one call of the reference's label path -> the stored fields of the case"""
    (ih, iw), n = sensor, len(raw)
    rec = dict(draws=[], dsize=None)

    def batch_resize(image, dsize, interpolation):
        rec['dsize'] = (int(dsize[0]), int(dsize[1]))
        return np.zeros((image.shape[0], dsize[1], dsize[0], image.shape[3]))

    def rand(a=0, b=1):
        rec['draws'].append(np.random.rand())
        return rec['draws'][-1] * (b - a) + a
    me = types.SimpleNamespace(batch_resize=batch_resize, rand=rand, letterbox_image=(branch != 2), format='cxcywh')
    numbered = np.concatenate([np.asarray(raw, dtype=np.float32).reshape(-1, 5), np.arange(n, dtype=np.float32)[:, None]], axis=1)
    np.random.seed(seed)
    frames, out = Dataset.get_random_data(me, np.zeros((1, 2, ih, iw)), numbered, input_shape=canvas, random=(branch == 0))
    assert frames.shape == (1, 2) + tuple(canvas) and out.dtype == np.float32 and len(rec['draws']) == (6 if branch == 0 else 0)
    # the permutation: the same shuffle of the row numbers from the same state
    np.random.seed(seed)
    for _ in rec['draws']:
        np.random.rand()
    perm = np.arange(n, dtype=np.int64)
    if n > 0:
        np.random.shuffle(perm)
    rows = out[:, 5].astype(np.int64).reshape(-1)
    assert [r for r in perm if r in set(rows.tolist())] == rows.tolist(), 'the survivors do not follow the replayed permutation'
    boxes = np.ascontiguousarray(out[:, :5]).reshape(-1, 5)
    _, targets = Transform()(frames, Dataset.reformat(me, boxes.copy()), canvas)
    assert targets.shape == (50, 5) and targets.dtype == np.float32
    return dict(raw=np.asarray(raw, dtype=np.float32).reshape(-1, 5), sensor=np.asarray(sensor, np.int64), canvas=np.asarray(canvas, np.int64),
                branch=np.asarray(branch, np.int64), draws=np.asarray(rec['draws'], np.float64), dsize=np.asarray(rec['dsize'], np.int64),
                perm=perm, boxes=boxes, rows=rows, targets=targets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of an EAS-SNN checkout (holds yolox/data/datasets/gen1.py)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'gen1_labels.npz'))
    args = ap.parse_args()
    Dataset, Transform = load_reference(args.reference)
    cases, names = [], []
    for gname, (sensor, canvas) in GEOMETRIES.items():
        for bname, raw in box_sets(*sensor).items():
            # the random branch twice: the first seeds (counted up from a fixed start) whose flip coin falls either way
            want, seed = {0: 'noflip', 1: 'flip'}, 100 * len(names)
            while want:
                case = run_case(Dataset, Transform, raw, sensor, canvas, 0, seed)
                flip = int(case['draws'][5] < .5)
                if flip in want:
                    names.append(f'{gname}_{bname}_{want.pop(flip)}')
                    cases.append(case)
                seed += 1
            for branch, tag in ((1, 'letterbox'), (2, 'resize')):
                names.append(f'{gname}_{bname}_{tag}')
                cases.append(run_case(Dataset, Transform, raw, sensor, canvas, branch, 7 + len(names)))
            kept = [len(c['rows']) for c in cases[-4:]]
            print(f'{gname} {bname}: {len(raw)} boxes, survivors {kept}')
            if bname == 'many':
                assert kept == [70] * 4, 'the 70 boxes are meant to survive every draw'
    # one array per field (an archive member per case and field would cost more than the data)
    out = {k: np.stack([c[k] for c in cases]) for k in ('sensor', 'canvas', 'branch', 'dsize', 'targets')}
    out['draws'] = np.stack([c['draws'] if len(c['draws']) else np.zeros(6) for c in cases])
    out['raw'], out['perm'] = np.concatenate([c['raw'] for c in cases]), np.concatenate([c['perm'] for c in cases])
    out['raw_offsets'] = np.cumsum([0] + [len(c['raw']) for c in cases]).astype(np.int64)
    out['boxes'], out['rows'] = np.concatenate([c['boxes'] for c in cases]), np.concatenate([c['rows'] for c in cases])
    out['box_offsets'] = np.cumsum([0] + [len(c['rows']) for c in cases]).astype(np.int64)
    np.savez_compressed(args.out, names=np.array(names), **out)
    print(args.out, os.path.getsize(args.out), 'bytes')
    assert os.path.getsize(args.out) < 64 * 1024


if __name__ == '__main__':
    main()
