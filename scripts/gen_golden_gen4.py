"""Writes tests/golden/gen4_front.npz: synthetic 1 Mpx labels and what the REFERENCE's own ``RVTGEN4Dataset.extract_labels`` (with its
``rescale`` closure, down_sample_factor 1 and 2) and ``__getitem__`` (the ``raw_bboxes`` it hands to get_random_data) make of them.

    python scripts/gen_golden_gen4.py --reference /path/to/EAS-SNN [--out tests/golden/gen4_front.npz]

yolox/data/datasets/rvt_gen4.py is loaded by file location under its package name, next to the real yolox/utils/util.py; everything else
it imports (cv2, h5py, loguru, tqdm, the dataset wrappers, yolox.utils.boxes, the psee loader, the cache) is an empty stand-in.
``extract_labels`` runs unbound on a ``SimpleNamespace(img_size, down_sample_factor)`` over a temporary ``<stream>/labels_v2`` directory
(real ``labels.npz`` / ``timestamps_us.npy`` files); ``__getitem__`` runs unbound on a namespace whose ``resolve_index`` and
``get_sample_resp`` are the reference's and whose ``generate_slices`` / ``get_random_data`` / ``target_transform`` are stand-ins that
record the boxes they are given (the representations are pinned elsewhere: tests/golden/stacked_hist.npz).  No bytecode is written into
the reference tree.  Only data is stored: ``labels`` float32 [L, 7] (t, x, y, w, h, class_id, class_confidence: the input),
``objframe_idx_2_label_idx`` int64, ``img_size``, and per factor f in (1, 2): ``dsf<f>/rows`` float32 [L', 7] with ``dsf<f>/offsets``
int64 [frames + 1] (the rows of every object frame after ``rescale``) and ``dsf<f>/raw_boxes`` float32 [L', 5]."""
import argparse
import importlib.util
import os
import shutil
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True

IMG_SIZE = (360, 640)
FIELDS = ('t', 'x', 'y', 'w', 'h', 'class_id', 'class_confidence')


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
    for name in ('cv2', 'h5py', 'loguru', 'tqdm', 'pycocotools', 'pycocotools.coco', 'yolox', 'yolox.data', 'yolox.data.datasets',
                 'yolox.data.datasets.datasets_wrapper', 'yolox.data.datasets.gen4_classes', 'yolox.utils', 'yolox.utils.boxes',
                 'yolox.utils.psee_loader', 'yolox.utils.psee_loader.io', 'yolox.utils.psee_loader.io.psee_loader', 'yolox.utils.cache'):
        sys.modules[name] = _Stub(name)
    try:
        import PIL  # noqa: F401
    except ImportError:
        sys.modules['PIL'] = _Stub('PIL')
    _load('yolox.utils.util', os.path.join(root, 'yolox', 'utils', 'util.py'))
    return _load('yolox.data.datasets.rvt_gen4', os.path.join(root, 'yolox', 'data', 'datasets', 'rvt_gen4.py')).RVTGEN4Dataset


def make_labels():
    """rows (t, x, y, w, h, class_id, class_confidence) in the 720 x 1280 coordinates the stored labels have, per object frame"""
    frames = [
        # frame 0: inside; across the right, bottom and left / top borders; odd coordinates (halves after the factor 2)
        [(100, 200, 150, 81, 61, 0, 1.0), (100, 1201, 333, 157, 99, 1, 0.9), (100, 640, 650, 90, 120, 2, 0.8), (100, -35, -12, 100, 77, 0, 0.7),
         (100, 3, 5, 7, 9, 1, 0.6)],
        # frame 1: boxes that lose their area after the clip (beyond the right border, above the top border, on the last column), one that stays
        [(200, 1290, 100, 50, 50, 0, 1.0), (200, 300, -80, 60, 70, 1, 1.0), (200, 1279, 10, 40, 40, 2, 0.5), (200, 500, 400, 33, 47, 2, 1.0)],
        # frame 2: no object
        [],
        # frame 3, the last one: the open-ended slice
        [(400, 17, 701, 45, 60, 1, 0.75), (400, 1000, 20, 279, 699, 0, 1.0)],
    ]
    rows = np.array([r for f in frames for r in f], dtype=np.float64)
    first = np.cumsum([0] + [len(f) for f in frames])[:-1].astype(np.int64)
    times = np.array([100, 200, 300, 400], dtype=np.int64)
    return rows, first, times


def write_stream(root, rows, first, times):
    label_dir = os.path.join(root, 'stream_a', 'labels_v2')
    os.makedirs(label_dir)
    dtype = np.dtype([('t', '<u8'), ('x', '<f4'), ('y', '<f4'), ('w', '<f4'), ('h', '<f4'), ('class_id', 'u1'), ('class_confidence', '<f4')])
    lab = np.zeros(len(rows), dtype=dtype)
    for k, name in enumerate(FIELDS):
        lab[name] = rows[:, k]
    np.savez(os.path.join(label_dir, 'labels.npz'), labels=lab, objframe_idx_2_label_idx=first)
    np.save(os.path.join(label_dir, 'timestamps_us.npy'), times)


def run_reference(Dataset, root, factor, num_slice=4):
    me = types.SimpleNamespace(img_size=IMG_SIZE, down_sample_factor=factor)
    files, labels, label_times = Dataset.extract_labels(me, [root])
    assert len(files) == 1 and len(labels[0]) == len(label_times[0])
    seen = []
    item_ns = types.SimpleNamespace(
        files=files, labels=labels, label_times=label_times, img_size=IMG_SIZE, input_size=IMG_SIZE, random_aug=False, map_val=True,
        end_idx=np.array([len(lab) for lab in labels]).cumsum(), slice_args=dict(num_slice=num_slice, aggregation='event_sum'),
        generate_slices=lambda file, time, n, method: np.zeros((1, n, 2) + IMG_SIZE),
        reformat=lambda boxes: boxes, target_transform=lambda frames, boxes, size: (frames, boxes))

    def get_random_data(frames, bboxes, input_shape, random=True):
        seen.append(np.array(bboxes))
        return frames, bboxes
    item_ns.get_random_data = get_random_data
    for m in ('resolve_index', 'get_sample_resp'):
        setattr(item_ns, m, types.MethodType(getattr(Dataset, m), item_ns))
    item_ns.sample_names = [item_ns.get_sample_resp(0, t) for t in range(len(labels[0]))]
    for item in range(len(labels[0])):
        Dataset.__getitem__(item_ns, item)
    assert len(seen) == len(labels[0])
    return labels[0], seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of an EAS-SNN checkout (holds yolox/data/datasets/rvt_gen4.py)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'gen4_front.npz'))
    args = ap.parse_args()
    Dataset = load_reference(args.reference)
    rows, first, times = make_labels()
    out = {'labels': rows.astype(np.float32), 'objframe_idx_2_label_idx': first, 'img_size': np.asarray(IMG_SIZE, np.int64)}
    for factor in (1, 2):
        root = tempfile.mkdtemp(prefix='eas_gen4_')
        try:
            write_stream(root, rows, first, times)
            frames, boxes = run_reference(Dataset, root, factor)
        finally:
            shutil.rmtree(root)
        assert all(f.dtype == np.float32 and f.shape[1:] == (7,) for f in frames) and all(b.dtype == np.float32 for b in boxes)
        out[f'dsf{factor}/rows'] = np.concatenate(frames).astype(np.float32)
        out[f'dsf{factor}/offsets'] = np.cumsum([0] + [len(f) for f in frames]).astype(np.int64)
        out[f'dsf{factor}/raw_boxes'] = np.concatenate([b.reshape(-1, 5) for b in boxes]).astype(np.float32)
        print(f'down_sample_factor {factor}: rows per object frame {[len(f) for f in frames]}')
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
