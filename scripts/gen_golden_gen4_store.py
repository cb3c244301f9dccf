"""Writes tests/golden/gen4_store.npz: two small synthetic 1 Mpx streams on disk and what the REFERENCE's own ``RVTGEN4Dataset`` makes of them
-- ``extract_labels``, ``resolve_index``, ``get_sample_resp``, ``generate_slices(..., method='event_sum')`` and the ``raw_bboxes`` of
``__getitem__`` -- with ``num_slice`` 3 and ``down_sample_factor`` 2: what ``data.Gen4Store`` has to reproduce.

    python scripts/gen_golden_gen4_store.py --reference /path/to/EAS-SNN [--out tests/golden/gen4_store.npz]

yolox/data/datasets/rvt_gen4.py is loaded as scripts/gen_golden_gen4.py loads it (``load_reference``: by file location, its imports empty
stand-ins).  The one difference: the ``h5py`` stand-in gets a ``File`` whose ``['data']`` serves the numpy array this script saved beside
the ``.h5`` path, so the reference's own read (``h5f['data'][max(start_idx, 0):end_idx]``) runs.  The streams: sensor 12 x 16, nbins 10, 7
and 5 representations; object frames on a subset of them, the first early enough that ``start_idx < 0``, one without boxes; boxes across
every border in the 24 x 32 coordinates of the stored labels.  ``__getitem__`` runs unbound on a namespace whose ``resolve_index``,
``get_sample_resp`` and ``generate_slices`` are the reference's and whose ``get_random_data`` records the slices and boxes it is given.

Only data is stored: per stream i ``s<i>/repr`` u8 [r, 20, 12, 16], ``s<i>/obj2repr``, ``s<i>/labels`` float32 [L, 7] (t, x, y, w, h,
class_id, class_confidence), ``s<i>/obj2label``, ``s<i>/label_times``; ``stream_names`` in the order the reference listed them;
``sample_names``; ``index_file`` / ``index_time`` (resolve_index of every flat index); ``slices`` float64 [N, 1, 3, 2, 12, 16];
``raw_boxes`` float32 [L', 5] with ``raw_offsets`` int64 [N + 1]."""
import argparse
import os
import shutil
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_gen4 import FIELDS, load_reference  # noqa: E402

SENSOR, NBINS, NUM_SLICE, FACTOR = (12, 16), 10, 3, 2
REP_NAME = 'stacked_histogram_dt=50_nbins=10'
LABEL_DTYPE = np.dtype([('t', '<u8'), ('x', '<f4'), ('y', '<f4'), ('w', '<f4'), ('h', '<f4'), ('class_id', 'u1'), ('class_confidence', '<f4')])


class ArrayFile:
    """``h5py.File(path, 'r')`` over ``<path>.npy``"""

    def __init__(self, path, mode='r'):
        self.data = {'data': np.load(path + '.npy')}

    def __enter__(self):
        return self.data

    def __exit__(self, *exc):
        return False


def make_streams():
    """[(name, repr u8 [r, 20, 12, 16], obj2repr, label rows float64 [L, 7], obj2label, label_times)]"""
    rng = np.random.default_rng(7)
    out = []
    frames_a = [
        # object frame 0 on representation 1: start_idx = 1 + 1 - 3 < 0; inside, across the right and the bottom border
        [(150, 4, 3, 9, 7, 0, 1.0), (150, 25, 6, 11, 8, 1, 0.9), (150, 10, 19, 6, 9, 2, 0.8)],
        # object frame 1: no object
        [],
        # object frame 2: across the left and the top border, odd coordinates (halves after the factor 2)
        [(350, -5, 8, 12, 7, 0, 0.7), (350, 13, -4, 7, 11, 1, 0.6)],
        # object frame 3, the last one (open-ended): one that loses its area after the clip, one that stays
        [(450, 33, 2, 5, 5, 2, 1.0), (450, 1, 1, 29, 21, 0, 1.0)],
    ]
    frames_b = [
        [(1200, 7, 5, 8, 8, 1, 1.0)],
        [(1250, 20, 15, 14, 12, 2, 0.5), (1250, -3, -2, 9, 9, 0, 1.0), (1250, 2, 17, 5, 3, 1, 1.0)],
        [(1300, 15, 10, 3, 9, 0, 1.0)],
    ]
    for name, r, obj2repr, frames in (('stream_a', 7, [1, 2, 4, 6], frames_a), ('stream_b', 5, [2, 3, 4], frames_b)):
        rep = np.minimum(rng.poisson(0.6, size=(r, 2 * NBINS) + SENSOR), 255).astype(np.uint8)
        rep[r - 1, :, 5, 9] = 255                        # a pixel saturated in every bin of both polarities: sum 2550
        rows = np.array([x for f in frames for x in f], dtype=np.float64).reshape(-1, 7)
        first = np.cumsum([0] + [len(f) for f in frames])[:-1].astype(np.int64)
        times = np.array([f[0][0] if f else 250 for f in frames], dtype=np.int64)
        out.append((name, rep, np.asarray(obj2repr, dtype=np.int64), rows, first, times))
    return out


def write_stream(root, name, rep, obj2repr, rows, first, times):
    label_dir = os.path.join(root, name, 'labels_v2')
    rep_dir = os.path.join(root, name, 'event_representations_v2', REP_NAME)
    os.makedirs(label_dir)
    os.makedirs(rep_dir)
    lab = np.zeros(len(rows), dtype=LABEL_DTYPE)
    for k, field in enumerate(FIELDS):
        lab[field] = rows[:, k]
    np.savez(os.path.join(label_dir, 'labels.npz'), labels=lab, objframe_idx_2_label_idx=first)
    np.save(os.path.join(label_dir, 'timestamps_us.npy'), times)
    np.save(os.path.join(rep_dir, 'objframe_idx_2_repr_idx.npy'), obj2repr)
    np.save(os.path.join(rep_dir, 'timestamps_us.npy'), 50 * (np.arange(len(rep), dtype=np.int64) + 1))
    np.save(os.path.join(rep_dir, 'event_representations_ds2_nearest.h5.npy'), rep)


def run_reference(Dataset, root):
    me = types.SimpleNamespace(img_size=SENSOR, down_sample_factor=FACTOR)
    files, labels, label_times = Dataset.extract_labels(me, [root])
    seen = []
    ns = types.SimpleNamespace(files=files, labels=labels, label_times=label_times, img_size=SENSOR, input_size=SENSOR, random_aug=False, map_val=True,
                               rep_name=REP_NAME, end_idx=np.array([len(lab) for lab in labels]).cumsum(),
                               slice_args=dict(num_slice=NUM_SLICE, aggregation='event_sum'), reformat=lambda boxes: boxes,
                               target_transform=lambda frames, boxes, size: (frames, boxes))

    def get_random_data(frames, bboxes, input_shape, random=True):
        seen.append((np.array(frames), np.array(bboxes)))
        return frames, bboxes
    ns.get_random_data = get_random_data
    for m in ('resolve_index', 'get_sample_resp', 'generate_slices'):
        setattr(ns, m, types.MethodType(getattr(Dataset, m), ns))
    n = int(ns.end_idx[-1])
    index = [ns.resolve_index(i) for i in range(n)]
    ns.sample_names = [ns.get_sample_resp(f, t) for f, t in index]
    for item in range(n):
        Dataset.__getitem__(ns, item)
    assert len(seen) == n
    return files, index, ns.sample_names, seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of an EAS-SNN checkout (holds yolox/data/datasets/rvt_gen4.py)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'gen4_store.npz'))
    args = ap.parse_args()
    Dataset = load_reference(args.reference)
    sys.modules['h5py'].File = ArrayFile
    streams = {s[0]: s for s in make_streams()}
    root = tempfile.mkdtemp(prefix='eas_gen4_store_')
    try:
        for s in streams.values():
            write_stream(root, *s)
        files, index, names, seen = run_reference(Dataset, root)
    finally:
        shutil.rmtree(root)
    order = [os.path.basename(f) for f in files]
    out = {'stream_names': np.array(order), 'sample_names': np.array(names), 'index_file': np.array([int(f) for f, _ in index], dtype=np.int64),
           'index_time': np.array([int(t) for _, t in index], dtype=np.int64), 'sensor': np.asarray(SENSOR, np.int64),
           'num_slice': np.int64(NUM_SLICE), 'nbins': np.int64(NBINS), 'down_sample_factor': np.int64(FACTOR)}
    for i, name in enumerate(order):
        _, rep, obj2repr, rows, first, times = streams[name]
        out.update({f's{i}/repr': rep, f's{i}/obj2repr': obj2repr, f's{i}/labels': rows.astype(np.float32), f's{i}/obj2label': first,
                    f's{i}/label_times': times})
    slices = np.stack([f.reshape(1, NUM_SLICE, 2, *SENSOR) for f, _ in seen])
    assert slices.dtype == np.float64 and all(b.dtype == np.float32 for _, b in seen)
    out['slices'] = slices
    out['raw_boxes'] = np.concatenate([b.reshape(-1, 5) for _, b in seen]).astype(np.float32)
    out['raw_offsets'] = np.cumsum([0] + [len(b.reshape(-1, 5)) for _, b in seen]).astype(np.int64)
    print('samples', names, 'boxes per sample', np.diff(out['raw_offsets']).tolist(), 'young', [int((s[0, 0] == 0).all()) for s in slices])
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
