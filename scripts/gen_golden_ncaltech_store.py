"""Writes tests/golden/ncaltech_store.npz: a tiny N-Caltech101 tree and what the REFERENCE's own dataset class makes of it -- ``NCaltech``'s
file list, ``read_annotation``, ``get_cls_names``, ``read_sample_name``, and the label path ``get_random_data(random=True)`` ->
``reformat('cxcywh')`` -> ``EventTrainTransform``, and the ``map_val`` labels (``reformat('xywh')`` -> ``EventValTransform``).

    python scripts/gen_golden_ncaltech_store.py --reference /path/to/EAS-SNN [--out tests/golden/ncaltech_store.npz]

yolox/data/datasets/ncaltech.py is loaded by file location under its package name with empty stand-ins for what it imports, except
yolox/utils/boxes.py (loaded for real, ``torchvision`` stubbed) and yolox/data/event_data_augment.py (the two transforms, loaded for real).
The tree is written into a temporary directory: ``Caltech101/<class>/`` directories (``BACKGROUND_Google`` among them; the recordings
themselves are never opened by what runs here, so none are written), ``Caltech101_annotations/<class>/annotation_*.bin`` and ``train.txt``,
which lists a ``BACKGROUND_Google`` sample too.  A real ``NCaltech`` object is built on it; its ``batch_resize`` is replaced by one that
returns zeros of the asked size and records ``dsize``, its ``rand`` by one that calls ``np.random.rand`` as the reference's does and records
each draw.  The script asserts that ``np.random.shuffle`` of the sample's single box consumes no random state (``shuffle_draws`` = 0: a
loader that replays the reference's draws has none to make for the box).  No bytecode is written into the reference tree.

Only data is stored: ``lines`` (train.txt), ``class_dirs`` (the listing of Caltech101/), ``label_paths`` of the N kept samples with their
byte images ``ann_bytes`` / ``ann_offsets`` [N + 1]; ``boxes`` int64 [N, 4] and ``class_idx`` int64 [N] (read_annotation), ``class_names``,
``sample_names``; ``val_labels`` float64 [N, 5] rows (x, y, w, h, class); ``geometries`` with ``sensor`` (ih, iw) and ``canvas`` (h, w); and
the C cases (geometry x sample x flip coin): ``case_geometry``, ``case_sample``, ``draws`` float64 [C, 6], ``dsize`` (nw, nh), ``targets``
float32 [C, 50, 5]."""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True

GEOMETRIES = {'ncaltech': ((180, 240), (192, 256)), 'small': ((36, 48), (64, 64))}
BACKGROUND = 'BACKGROUND_Google'
# (class, stem number, box contour [2, n] (x row, y row), object contour [2, m]): on the 180 x 240 sensor one box inside, one that reaches
# past it, one with a negative corner, one a pixel wide that no draw lets survive; two that also lie inside the 36 x 48 sensor
SAMPLES = [
    ('airplanes', 1, [[60, 160, 160, 60, 60], [50, 50, 130, 130, 50]], [[70, 90, 120], [60, 100, 80]]),
    ('airplanes', 7, [[150, 260, 260, 150, 150], [100, 100, 200, 200, 100]], [[0], [0]]),
    ('Faces_easy', 3, [[-8, 100, 100, -8, -8], [-4, -4, 90, 90, -4]], [[5, 6, 7, 8], [1, 2, 3, 4]]),
    ('Faces_easy', 12, [[100, 101, 101, 100, 100], [80, 80, 140, 140, 80]], [[3], [4]]),
    ('butterfly', 2, [[30, 5, 30, 5], [25, 25, 4, 4]], [[9, 9], [8, 8]]),                       # an open contour, corners in another order
    ('butterfly', 5, [[-3, 40, 40, -3, -3], [10, 10, 30, 30, 10]], [[1, 2], [3, 4]]),
]


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
    for name in ('cv2', 'loguru', 'torchvision', 'pycocotools', 'pycocotools.coco', 'yolox', 'yolox.data', 'yolox.data.dataloading',
                 'yolox.data.datasets', 'yolox.data.datasets.datasets_wrapper', 'yolox.utils', 'yolox.utils.util', 'yolox.utils.event_reps'):
        sys.modules[name] = _Stub(name)
    boxes = _load('yolox.utils.boxes', os.path.join(root, 'yolox', 'utils', 'boxes.py'))
    sys.modules['yolox.utils'].xyxy2cxcywh, sys.modules['yolox.utils'].normalize_box = boxes.xyxy2cxcywh, boxes.normalize_box
    dataset = _load('yolox.data.datasets.ncaltech', os.path.join(root, 'yolox', 'data', 'datasets', 'ncaltech.py')).NCaltech
    augment = _load('yolox.data.event_data_augment', os.path.join(root, 'yolox', 'data', 'event_data_augment.py'))
    return dataset, augment.TrainTransform, augment.ValTransform


def annotation_image(box, obj):
    """the byte image of an annotation file: (rows, cols) int16 and the column-major int16 values, for the box contour, then the object's"""
    out = []
    for a in (np.asarray(box, dtype='<i2'), np.asarray(obj, dtype='<i2')):
        out += [np.asarray(a.shape, dtype='<i2').tobytes(), a.reshape(-1, order='F').tobytes()]
    return b''.join(out)


def write_tree(root):
    """-> the lines of train.txt; the BACKGROUND_Google sample stands in the middle of the list"""
    lines = []
    for cls in sorted({s[0] for s in SAMPLES} | {BACKGROUND}):
        os.makedirs(os.path.join(root, 'Caltech101', cls))
        os.makedirs(os.path.join(root, 'Caltech101_annotations', cls))
    for cls, k, box, obj in SAMPLES:
        label = f'Caltech101_annotations/{cls}/annotation_{k:04d}.bin'
        with open(os.path.join(root, label), 'wb') as f:
            f.write(annotation_image(box, obj))
        lines.append(f'Caltech101/{cls}/image_{k:04d}.bin {label}\n')
    label = f'Caltech101_annotations/{BACKGROUND}/annotation_0001.bin'
    with open(os.path.join(root, label), 'wb') as f:
        f.write(annotation_image([[1, 2], [3, 4]], [[0], [0]]))
    lines.insert(3, f'Caltech101/{BACKGROUND}/image_0001.bin {label}\n')
    with open(os.path.join(root, 'train.txt'), 'w') as f:
        f.writelines(lines)
    return lines


def run_case(ds, raw, sensor, canvas, seed):
    """one call of the reference's training label path -> (draws, dsize, targets)"""
    rec = dict(draws=[], dsize=None)

    def batch_resize(image, dsize, interpolation):
        rec['dsize'] = (int(dsize[0]), int(dsize[1]))
        return np.zeros((image.shape[0], dsize[1], dsize[0], image.shape[3]))

    def rand(a=0, b=1):
        rec['draws'].append(np.random.rand())
        return rec['draws'][-1] * (b - a) + a
    ds.batch_resize, ds.rand = batch_resize, rand
    np.random.seed(seed)
    frames, boxes = ds.get_random_data(np.zeros((1, 2) + tuple(sensor)), raw.copy(), input_shape=canvas, random=True)
    after = np.random.rand()
    assert frames.shape == (1, 2) + tuple(canvas) and boxes.dtype == np.float32 and len(rec['draws']) == 6
    # the state behind the call is the state behind six draws: the shuffle of the single box drew nothing
    np.random.seed(seed)
    assert [np.random.rand() for _ in range(6)] == rec['draws'] and np.random.rand() == after, 'the box shuffle consumed random state'
    _, targets = ds.target_transform(frames, ds.reformat(boxes), canvas)
    assert targets.shape == (50, 5) and targets.dtype == np.float32
    return np.asarray(rec['draws'], np.float64), np.asarray(rec['dsize'], np.int64), targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of an EAS-SNN checkout (holds yolox/data/datasets/ncaltech.py)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'ncaltech_store.npz'))
    args = ap.parse_args()
    Dataset, TrainTransform, ValTransform = load_reference(args.reference)
    slice_args = dict(num_slice=1, overlap=0, aggregation='micro_sum', micro_slice=3, measure='count')
    state = np.random.get_state()[1].copy()
    np.random.shuffle(np.zeros((1, 5)))
    assert np.array_equal(state, np.random.get_state()[1])
    out = {}
    with tempfile.TemporaryDirectory() as root:
        out['lines'] = np.array([ln.strip() for ln in write_tree(root)])
        out['class_dirs'] = np.array(sorted(os.listdir(os.path.join(root, 'Caltech101'))))
        (sensor, canvas) = GEOMETRIES['ncaltech']
        ds = Dataset(root, canvas, type='train', class_names=None, img_size=sensor, random_aug=True,
                     target_transform=TrainTransform(box_norm=False), **slice_args)
        val = Dataset(root, canvas, type='train', class_names=None, img_size=sensor, map_val=True, letterbox_image=True, format='xywh',
                      random_aug=False, target_transform=ValTransform(box_norm=False), **slice_args)
        n = len(ds.file_list)
        assert n == len(SAMPLES) and len(ds) == n
        label_paths = [ln.strip().split(' ')[1] for ln in ds.file_list]
        images = [np.fromfile(os.path.join(root, p), dtype=np.uint8) for p in label_paths]
        read = [ds.read_annotation(os.path.join(root, p)) for p in label_paths]
        out['label_paths'] = np.array(label_paths)
        out['ann_bytes'], out['ann_offsets'] = np.concatenate(images), np.cumsum([0] + [len(a) for a in images]).astype(np.int64)
        out['boxes'] = np.array([[int(v) for v in r[0]] for r in read], dtype=np.int64)
        out['class_idx'] = np.array([int(r[2]) for r in read], dtype=np.int64)
        out['class_names'], out['sample_names'] = np.array(ds.class_names), np.array(ds.read_sample_name())
        assert list(out['sample_names']) == list(ds.sample_names)
        raws = [np.array([list(r[0]) + [r[2]]], dtype=np.float64) for r in read]               # raw_bboxes of __getitem__
        out['val_labels'] = np.concatenate([val.target_transform(None, val.reformat(r.copy()), canvas)[1] for r in raws]).astype(np.float64)
        cases = []
        for g, (gname, (sensor, canvas)) in enumerate(GEOMETRIES.items()):
            survivors = []
            for i, raw in enumerate(raws):
                # the first seeds (counted up from a fixed start) whose flip coin falls either way
                want, seed = {0, 1}, 1000 * g + 100 * i
                while want:
                    draws, dsize, targets = run_case(ds, raw, sensor, canvas, seed)
                    flip = int(draws[5] < .5)
                    if flip in want:
                        want.discard(flip)
                        cases.append((g, i, draws, dsize, targets))
                        survivors.append(int(targets.any()))
                    seed += 1
            print(f'{gname}: sensor {sensor} canvas {canvas}: survivors per case {survivors}')
    assert any(not c[4].any() for c in cases) and any(c[4].any() for c in cases)
    out['geometries'] = np.array(list(GEOMETRIES))
    out['sensor'] = np.array([g[0] for g in GEOMETRIES.values()], dtype=np.int64)
    out['canvas'] = np.array([g[1] for g in GEOMETRIES.values()], dtype=np.int64)
    out['case_geometry'], out['case_sample'] = (np.array([c[k] for c in cases], dtype=np.int64) for k in (0, 1))
    out['draws'], out['dsize'], out['targets'] = (np.stack([c[k] for c in cases]) for k in (2, 3, 4))
    out['shuffle_draws'] = np.asarray(0, dtype=np.int64)
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')
    assert os.path.getsize(args.out) < 64 * 1024


if __name__ == '__main__':
    main()
