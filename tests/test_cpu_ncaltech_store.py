"""CPU tests of N-Caltech101 training from recordings in HBM: the new entry points are declared and exported, the store's workspace does not
grow with the store, and the host side of ``NCaltechStore`` and its loaders -- annotation parser, file list, names, classes, box table, the
draws of an epoch -- against tests/golden/ncaltech_store.npz, recorded from the reference's own ``NCaltech`` class
(scripts/gen_golden_ncaltech_store.py).  Every value is an integer or a half: every comparison is exact."""
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, load_golden

import labels_ref
import eas_snn_amd
from eas_snn_amd import _lib, data

NEW = ['eas_atis_store_index_bytes', 'eas_atis_store_index', 'eas_atis_store_workspace_bytes', 'eas_atis_store_timesurface_workspace_bytes',
       'eas_event_histogram_atis_store', 'eas_event_timesurface_atis_store', 'eas_event_latest_surface_atis_store']


@pytest.fixture(scope='module')
def gold():
    return load_golden('ncaltech_store')


def test_new_symbols_are_declared_and_exported_at_abi_9():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'eas_hip.h')).read(), flags=re.S)
    lib = eas_snn_amd.hip_library()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', src), f'{name} is not declared in include/eas_hip.h'
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.eas_abi_version() == _lib.ABI_VERSION == 9


def test_store_workspace_takes_no_record_count():
    """heads (40 bytes per recording), slice rows (8 per macro slice) and, for the time surface, t_target (4 per macro slice), each part
    rounded up to 16 bytes: nothing that depends on the store"""
    lib = eas_snn_amd.hip_library()
    a16 = lambda v: (v + 15) // 16 * 16
    for query in ('eas_atis_store_workspace_bytes', 'eas_atis_store_timesurface_workspace_bytes'):
        assert len(_lib.PROTOTYPES[query][1]) == 2
    for B, Tl in ((1, 1), (64, 2)):
        count = a16(40 * B) + a16(8 * B * Tl)
        assert lib.eas_atis_store_workspace_bytes(B, Tl) == count
        assert lib.eas_atis_store_timesurface_workspace_bytes(B, Tl) == count + a16(4 * B * Tl)
        # the packed entries' workspace is the same plan behind an index of the buffer
        for nrec in (0, 1000):
            assert lib.eas_event_histogram_atis_workspace_bytes(nrec, B, Tl) == a16(lib.eas_atis_store_index_bytes(nrec)) + count
    assert [lib.eas_atis_store_workspace_bytes(1, 1), lib.eas_atis_store_workspace_bytes(64, 2)] == [64, 3584]
    assert [lib.eas_atis_store_timesurface_workspace_bytes(1, 1), lib.eas_atis_store_timesurface_workspace_bytes(64, 2)] == [80, 4096]
    assert [lib.eas_atis_store_index_bytes(n) for n in (0, 1, 256, 257)] == [4, 8, 8, 12]
    assert lib.eas_atis_store_workspace_bytes(0, 1) == 0 and lib.eas_atis_store_workspace_bytes(1, 0) == 0


def annotations(gold):
    off = gold['ann_offsets']
    return [gold['ann_bytes'][off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_annotation_parser_equals_the_reference_and_encode_round_trips(gold):
    images = annotations(gold)
    assert len(images) == 6
    for image, box in zip(images, gold['boxes']):
        assert data.parse_ncaltech_annotation(image) == tuple(int(v) for v in box)
        assert data.parse_ncaltech_annotation(image.tobytes()) == tuple(int(v) for v in box)
        again = data.encode_ncaltech_annotation(*box, contour=[(3, 4), (5, 6), (-7, 8)])
        assert again.dtype == np.uint8 and data.parse_ncaltech_annotation(again) == tuple(int(v) for v in box)
    # the object contour stands behind the box contour and is not looked at
    a, b = data.encode_ncaltech_annotation(-300, 2, 5, 700), data.encode_ncaltech_annotation(-300, 2, 5, 700, contour=[(9, 9)] * 4)
    assert len(b) == len(a) + 12 and data.parse_ncaltech_annotation(a) == data.parse_ncaltech_annotation(b) == (-300, 2, 5, 700)
    assert (gold['boxes'] < 0).any() and (gold['boxes'][:, 2] > 240).any()


def write_tree(root, gold):
    """the fixture's tree: train.txt, the class directories, the annotation images of the kept samples and a small recording per line"""
    lines = [str(ln) for ln in gold['lines']]
    for cls in gold['class_dirs']:
        os.makedirs(os.path.join(root, 'Caltech101', str(cls)))
        os.makedirs(os.path.join(root, 'Caltech101_annotations', str(cls)))
    with open(os.path.join(root, 'train.txt'), 'w') as f:
        f.writelines(ln + '\n' for ln in lines)
    for path, image in zip(gold['label_paths'], annotations(gold)):
        image.tofile(os.path.join(root, str(path)))
    sizes = {}
    for k, ln in enumerate(lines):
        n = 3 + 2 * k
        rec = data.encode_atis(20_000 + np.arange(n) * 5000, np.arange(n) % 16, np.arange(n) % 12, np.arange(n) % 2, overflow_before=[1] * (k % 3))
        rec.tofile(os.path.join(root, ln.split(' ')[0]))
        sizes[ln.split(' ')[0]] = len(rec) // 5
    return lines, sizes


@pytest.fixture(scope='module')
def store(gold, tmp_path_factory):
    root = str(tmp_path_factory.mktemp('ncaltech'))
    lines, sizes = write_tree(root, gold)
    return data.NCaltechStore.from_directory(root, 'train', 2, (-20_000, 0), 'cpu'), lines, sizes


def test_store_tables_names_and_classes_equal_the_reference(gold, store):
    s, lines, sizes = store
    kept = [ln for ln in lines if 'BACKGROUND_Google' not in ln]
    assert len(lines) == 7 and len(kept) == 6 == len(s)                          # the BACKGROUND_Google line is dropped
    assert s.sample_names == [str(n) for n in gold['sample_names']] and s.class_names == [str(n) for n in gold['class_names']]
    assert 'BACKGROUND_Google' in [str(c) for c in gold['class_dirs']] and 'BACKGROUND_Google' not in s.class_names
    assert s.host['boxes'].dtype == np.float32 and s.host['boxes'].shape == (6, 5)
    assert np.array_equal(s.host['boxes'][:, :4], gold['boxes']) and np.array_equal(s.host['boxes'][:, 4], gold['class_idx'])
    assert np.array_equal(s.host['group_start'], np.arange(7)) and s.host['group_start'].dtype == np.int64
    counts = [sizes[ln.split(' ')[0]] for ln in kept]
    assert np.array_equal(s.host['file_offsets'], np.cumsum([0] + counts)) and s.max_file_records == max(counts)
    assert s.records.dtype.is_floating_point is False and s.records.numel() == 5 * sum(counts) and s.Tl == 2 and s.window == (-20_000, 0)
    for k in s.host:
        assert np.array_equal(getattr(s, k).numpy(), s.host[k])
    # the evaluation's labels: xywh rows, untransformed
    for i in range(6):
        lab = s.raw_labels(i)
        assert lab.dtype == np.float32 and lab.shape == (1, 5) and np.array_equal(lab, gold['val_labels'][i:i + 1])
    # the same recordings handed over as tuples, classes taken from them
    recs = [(n.split('-')[0], n.split('-')[1], np.zeros(0, np.uint8), a) for n, a in zip(s.sample_names, annotations(gold))]
    recs.insert(2, ('BACKGROUND_Google', 'image_0001', np.zeros(5, np.uint8), annotations(gold)[0]))
    t = data.NCaltechStore(recs, 1, None, 'cpu')
    assert t.sample_names == s.sample_names and t.class_names == s.class_names and np.array_equal(t.host['boxes'], s.host['boxes'])
    assert t.max_file_records == 0 and t.window is None and t.index is None
    with pytest.raises(ValueError):
        data.NCaltechStore([('a', 'b', np.zeros(7, np.uint8), annotations(gold)[0])], 1, None, 'cpu')


def test_targets_of_the_recorded_draws_equal_the_reference(gold, store):
    s = store[0]
    assert int(gold['shuffle_draws']) == 0 and len(gold['draws']) == 24
    flips, kept = set(), 0
    for g, i, draws, dsize, want in zip(gold['case_geometry'], gold['case_sample'], gold['draws'], gold['dsize'], gold['targets']):
        (ih, iw), (h, w) = (int(v) for v in gold['sensor'][g]), (int(v) for v in gold['canvas'][g])
        rng = labels_ref.Replay(draws)
        par = data.jitter_params(ih, iw, h, w, jitter=.1, rng=rng)
        assert not rng.draws and par[:2] == tuple(int(v) for v in dsize)
        got, count, flags = labels_ref.targets(s.host['boxes'], s.host['group_start'], [int(i)], [par], ih, iw, h, w)
        assert np.array_equal(got[0], want) and flags[0] == 0 and count[0] == int(want.any())
        flips.add((int(g), int(i), par[4]))
        kept += int(count[0])
    assert len(flips) == 24 and 8 < kept < 24


def small_exp():
    return types.SimpleNamespace(Tm=3, Tl=2, input_size=(192, 256), test_size=(192, 256), num_classes=3, window=-20)


def test_batches_are_a_function_of_seed_and_epoch(store):
    s = store[0]
    loader = data.NCaltechStoreLoader(small_exp(), 2, store=s, seed=3)
    assert len(loader) == 3 and len(loader.dataset) == 6 and loader.dataset.class_names == s.class_names
    assert loader.dataset.map_val and not loader.dataset.random_aug and loader.dataset.sample_names is s.sample_names
    a, b, c = loader.batches(0), loader.batches(0), loader.batches(1)
    same = lambda p, q: all(np.array_equal(u, v) for x, y in zip(p, q) for u, v in zip(x, y))
    assert same(a, b) and not same(a, c)
    assert not same(a, data.NCaltechStoreLoader(small_exp(), 2, store=s, seed=4).batches(0))
    assert sorted(np.concatenate([idx for idx, _ in a]).tolist()) == list(range(6))
    for idx, par in a:
        assert idx.dtype == np.int64 and idx.shape == (2,) and par.dtype == np.int32 and par.shape == (2, 5)
    with pytest.raises(ValueError):
        data.NCaltechStoreLoader(types.SimpleNamespace(Tm=3, input_size=(192, 256), aggregation='voxel_grid'), 2, store=s)


def test_params_follow_the_reference_draw_order(store):
    """a replayed RandomState: the epoch's permutation, then six uniform draws per sample and none for its single box"""
    s = store[0]
    loader = data.NCaltechStoreLoader(small_exp(), 3, store=s, seed=7)
    rs = np.random.RandomState((7 * 1_000_003 + 5) % (1 << 32))
    order = rs.permutation(6)
    for idx, par in loader.batches(5):
        assert np.array_equal(idx, order[:3])
        order = order[3:]
        for row in par:
            draws = [rs.rand() for _ in range(6)]
            assert tuple(int(v) for v in row) == data.jitter_params(180, 240, 192, 256, jitter=.1, rng=labels_ref.Replay(draws))
            assert 0.4 * 256 - 1 <= row[0] <= 256 and row[4] in (0, 1)
