"""Plain numpy checker of the 1 Mpx store (data.Gen4Store, eas_stacked_hist_bin_sums, eas_count_store_frames): the store tables written out
recording by recording as RVTGEN4Dataset builds its lists (extract_labels with its ``rescale``, resolve_index, get_sample_resp, the start
index of generate_slices; rvt_gen4.py:109-125, 246-248, 296-300, 365-407), and the bin sums as the reference's reshape and sum.  Frames
and targets come from the existing checkers: ``gen4_ref.frames`` on the UNSUMMED representations and ``labels_ref.targets``.
tests/test_cpu_hist_store.py pins all of it to tests/golden/gen4_store.npz, recorded from the reference (scripts/gen_golden_gen4_store.py)."""
import numpy as np

import gen4_ref
import labels_ref

FIELDS = ('t', 'x', 'y', 'w', 'h', 'class_id', 'class_confidence')


def fixture_recordings(g):
    """the recordings of tests/golden/gen4_store.npz (``g``: the loaded archive) as ``data.Gen4Store`` takes them, in the reference's order"""
    return [(str(name), g[f's{i}/repr'], g[f's{i}/obj2repr'], g[f's{i}/labels'], g[f's{i}/obj2label'], g[f's{i}/label_times'])
            for i, name in enumerate(g['stream_names'])]


def bin_sums(hist, nbins=10):
    """uint16 [n, 2, H, W]: generate_slices' ``reshape(n, 2, -1, H, W).sum(axis=2)`` (rvt_gen4.py:121-122)"""
    hist = np.asarray(hist)
    n, c, H, W = hist.shape
    assert c == 2 * nbins and hist.dtype == np.uint8
    s = hist.reshape(n, 2, nbins, H, W).sum(2)
    assert s.max(initial=0) <= 65535
    return s.astype(np.uint16)


def rows_of(label_rows):
    """float32 [L, 7] of a structured ``labels`` array, as extract_labels stacks its fields (rvt_gen4.py:395-396)"""
    if getattr(label_rows, 'dtype', None) is not None and label_rows.dtype.names:
        return np.stack([label_rows[k].astype('float32') for k in FIELDS], axis=-1).reshape(-1, 7)
    return np.array(label_rows, dtype=np.float32).reshape(-1, 7)


def rescaled_boxes(rows, factor, sensor_hw):
    """(x1, y1, x2, y2, class) float32 rows of one object frame: ``rescale`` (rvt_gen4.py:370-387) then ``raw_bboxes`` (:199-207)"""
    rows = np.array(rows, dtype=np.float32).reshape(-1, 7)
    m = 1.0 / factor
    if len(rows) and m != 1:
        h, w = sensor_hw
        x2, y2 = np.clip((rows[:, 1] + rows[:, 3]) * m, 0, w - 1), np.clip((rows[:, 2] + rows[:, 4]) * m, 0, h - 1)
        x1, y1 = np.clip(rows[:, 1] * m, 0, w - 1), np.clip(rows[:, 2] * m, 0, h - 1)
        rows[:, 3], rows[:, 4], rows[:, 1], rows[:, 2] = x2 - x1, y2 - y1, x1, y1
        rows = rows[(rows[:, 3] > 0) & (rows[:, 4] > 0)]
    return np.stack([rows[:, 1], rows[:, 2], rows[:, 1] + rows[:, 3], rows[:, 2] + rows[:, 4], rows[:, 5]], axis=-1).astype(np.float32)


def tables(recordings, num_slice, factor=2, sensor_hw=(360, 640)):
    """dict of the store's tables + ``sample_names`` + ``index`` ((file, time) of every flat index)"""
    rep_offsets, group_first, group_lo, boxes, group_start, names, index = [0], [], [], [], [0], [], []
    for f, (name, rep, obj2repr, label_rows, obj2label, label_times) in enumerate(recordings):
        rows = rows_of(label_rows)
        assert len(label_times) == len(obj2label), 'Label time is not consistent with the label'
        offset = rep_offsets[-1]
        rep_offsets.append(offset + len(rep))
        for k, a in enumerate(obj2label):
            mine = rows[a:] if k + 1 == len(obj2label) else rows[a:obj2label[k + 1]]
            box = rescaled_boxes(mine, factor, sensor_hw)
            boxes.append(box)
            group_start.append(group_start[-1] + len(box))
            group_first.append(offset + int(obj2repr[k]) + 1 - num_slice)          # end_idx - num_slice, in the store
            group_lo.append(offset)
            names.append(f'{name}_n{num_slice}_a{label_times[k]}')
            index.append((f, k))
    return dict(rep_offsets=np.array(rep_offsets, dtype=np.int64), group_first=np.array(group_first, dtype=np.int64),
                group_lo=np.array(group_lo, dtype=np.int64), boxes=np.concatenate(boxes).reshape(-1, 5).astype(np.float32),
                group_start=np.array(group_start, dtype=np.int64), sample_names=names, index=index)


def frames(recordings, tab, sample_idx, num_slice, Hc, Wc, nbins=10, params=None):
    """float32 [B, 1, num_slice, 2, Hc, Wc] of the samples ``sample_idx``: ``gen4_ref.frames`` on the unsummed representations back to back"""
    store = np.concatenate([np.asarray(r[1]) for r in recordings])
    idx = np.asarray(sample_idx, dtype=np.int64)
    return gen4_ref.frames(store, tab['group_first'][idx], num_slice, Hc, Wc, nbins=nbins, lo=tab['group_lo'][idx], params=params)[0]


def targets(tab, sample_idx, params, sensor_hw, canvas_hw, perm=None, max_labels=50):
    """(targets, count, flags) of ``labels_ref.targets`` on the checker's box table"""
    return labels_ref.targets(tab['boxes'], tab['group_start'], np.asarray(sample_idx, dtype=np.int64), params, *sensor_hw, *canvas_hw, perm=perm,
                              max_labels=max_labels)
