"""Plain numpy checker of the label kernel (eas_label_targets, include/eas_hip.h): ``data.transform_boxes`` -- the project's statement of the
box half of get_random_data -- on the rows a sample's ``perm`` picks, the centre form of ``xyxy2cxcywh`` in float32, the zero padding of
EventTrainTransform and the flag rules, sample by sample.  tests/test_cpu_gen1_store.py pins it to tests/golden/gen1_labels.npz, which was
recorded from the reference's own functions (scripts/gen_golden_gen1_labels.py), bit for bit."""
import numpy as np

from eas_snn_amd import data

FLAG_PERM, FLAG_ROWS, FLAG_GROUP = 1, 2, 4


class Replay:
    """an ``rng`` that hands out recorded draws"""

    def __init__(self, draws):
        self.draws = list(draws)

    def rand(self):
        return self.draws.pop(0)


def fixture_cases(g):
    """(name, fields) of every case of tests/golden/gen1_labels.npz (``g``: the loaded archive)"""
    ro, bo = g['raw_offsets'], g['box_offsets']
    for c, name in enumerate(str(n) for n in g['names']):
        yield name, dict(raw=g['raw'][ro[c]:ro[c + 1]], perm=g['perm'][ro[c]:ro[c + 1]], boxes=g['boxes'][bo[c]:bo[c + 1]],
                         rows=g['rows'][bo[c]:bo[c + 1]], sensor=tuple(int(v) for v in g['sensor'][c]), canvas=tuple(int(v) for v in g['canvas'][c]),
                         branch=int(g['branch'][c]), draws=g['draws'][c], dsize=tuple(int(v) for v in g['dsize'][c]), targets=g['targets'][c])


def case_params(case):
    """(nw, nh, dx, dy, flip) of a fixture case from its recorded draws, by the project's own functions"""
    (ih, iw), (h, w) = case['sensor'], case['canvas']
    if case['branch'] == 0:
        rng = Replay(case['draws'])
        par = data.jitter_params(ih, iw, h, w, jitter=.3, rng=rng)
        assert not rng.draws                                                    # six draws, all used
        return par
    return data.letterbox_params(ih, iw, h, w, letterbox=(case['branch'] == 1))


def picked_rows(n, perm_row):
    """(row numbers of a group of ``n`` rows in the order of ``perm_row`` -- None: identity --, flag bits)"""
    if perm_row is None:
        return list(range(n)), 0
    flags = FLAG_ROWS if n > len(perm_row) else 0
    rows = []
    for r in perm_row[:min(n, len(perm_row))]:
        if 0 <= int(r) < n:
            rows.append(int(r))
        else:
            flags |= FLAG_PERM
    return rows, flags


def sample_targets(raw, params, ih, iw, h, w, perm_row=None, max_labels=50):
    """(targets float32 [max_labels, 5] rows (cls, cx, cy, w, h), survivors before the cut, flag bits, boxes float32 [k, 5] after the
    transform) of one sample: ``raw`` float32 [n, 5] rows (x1, y1, x2, y2, class), ``params`` (nw, nh, dx, dy, flip)"""
    raw = np.asarray(raw, dtype=np.float32).reshape(-1, 5)
    rows, flags = picked_rows(len(raw), perm_row)
    box = data.transform_boxes(raw[rows], tuple(int(v) for v in params), ih, iw, h, w).reshape(-1, 5)
    assert box.dtype == np.float32
    t = np.zeros((max_labels, 5), dtype=np.float32)
    k = min(len(box), max_labels)
    bw, bh = box[:k, 2] - box[:k, 0], box[:k, 3] - box[:k, 1]                 # float32 throughout, as xyxy2cxcywh on the float32 rows
    t[:k, 0] = box[:k, 4]
    t[:k, 1], t[:k, 2] = box[:k, 0] + bw * np.float32(0.5), box[:k, 1] + bh * np.float32(0.5)
    t[:k, 3], t[:k, 4] = bw, bh
    return t, len(box), flags, box


def targets(boxes, group_start, group, params, ih, iw, h, w, perm=None, max_labels=50):
    """(targets float32 [B, max_labels, 5], count int32 [B], flags int32 [B]) as eas_label_targets defines them"""
    boxes, group_start = np.asarray(boxes, dtype=np.float32).reshape(-1, 5), np.asarray(group_start, dtype=np.int64)
    B, G = len(group), len(group_start) - 1
    out, count, flags = np.zeros((B, max_labels, 5), dtype=np.float32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b, g in enumerate(group):
        if not 0 <= int(g) < G:
            flags[b] = FLAG_GROUP
            continue
        raw = boxes[group_start[g]:group_start[g + 1]]
        out[b], count[b], flags[b], _ = sample_targets(raw, params[b], ih, iw, h, w, None if perm is None else perm[b], max_labels)
    return out, count, flags
