"""CPU-only tests of 1 Mpx training from recordings in HBM: ``eas_stacked_hist_bin_sums`` and ``eas_count_store_frames`` are declared, exported,
bound and refuse bad arguments before any launch; the numpy checker (tests/gen4_store_ref.py) equals tests/golden/gen4_store.npz -- recorded
from the reference's own ``extract_labels`` / ``resolve_index`` / ``get_sample_resp`` / ``generate_slices`` / ``__getitem__``
(scripts/gen_golden_gen4_store.py) -- exactly; the tables, names and sample order of ``data.Gen4Store`` on host tensors equal the
checker's, from a list and from directories; the draws of ``data.Gen4StoreLoader``; the experiment's ``train_input = 'hist_store'``."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import gen4_store_ref
import eas_snn_amd
from eas_snn_amd import data, ops

INVALID, UNSUPPORTED = -1, -2
TABLES = ('rep_offsets', 'group_first', 'group_lo', 'boxes', 'group_start')


@pytest.fixture(scope='module')
def golden():
    return load_golden('gen4_store')


@pytest.fixture(scope='module')
def recordings(golden):
    return gen4_store_ref.fixture_recordings(golden)


def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    eas_snn_amd._lib._bind_host_hip_runtime()
    handle = ctypes.CDLL(eas_snn_amd._lib.LIB_PATH)
    C = ctypes
    want = {'eas_stacked_hist_bin_sums': (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
            'eas_count_store_frames': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3)}
    for n, proto in want.items():
        assert n in declared and hasattr(handle, n) and eas_snn_amd._lib.PROTOTYPES[n] == proto
    assert sorted(eas_snn_amd._lib.PROTOTYPES) == sorted(declared)
    assert eas_snn_amd._lib.ABI_VERSION == 9 and eas_snn_amd.hip_library().eas_abi_version() == 9          # purely additive
    assert hasattr(ops, 'stacked_hist_bin_sums') and hasattr(ops, 'count_store_frames')
    for name in ('Gen4Store', 'hist_store_for', 'synth_gen4_recordings', 'Gen4StoreDataset', 'Gen4StoreLoader', 'Gen4StoreEvalLoader'):
        assert hasattr(data, name)


def test_bad_arguments_are_refused_before_any_launch():
    """every call below returns from the argument checks: no device is touched (the pointers are made-up addresses)"""
    lib = eas_snn_amd.hip_library()
    good = dict(hist=0x10000, n=3, nbins=10, H=18, W=32, sums=0x20000)

    def sums(**kw):
        a = dict(good, **kw)
        return lib.eas_stacked_hist_bin_sums(a['hist'], a['n'], a['nbins'], a['H'], a['W'], a['sums'], None)
    for kw in (dict(hist=None), dict(sums=None), dict(n=-1), dict(nbins=0), dict(H=0), dict(W=0), dict(hist=0x10004), dict(sums=0x20008),
               dict(sums=0x20001, W=30)):
        assert sums(**kw) == INVALID, kw
    assert sums(nbins=256) == UNSUPPORTED and sums(n=0) == 0 and sums(n=0, nbins=0) == INVALID
    assert sums(n=0, W=30, hist=0x10003, sums=0x20002) == 0                   # rows that are not 16-byte aligned: the element path asks for less
    good = dict(sums=0x10000, R=8, first=0x20000, lo=0x30000, params=0x40000, B=2, Tm=3, H=18, W=32, Hc=32, Wc=48, out=0x50000, flags=0x60000)

    def frames(**kw):
        a = dict(good, **kw)
        return lib.eas_count_store_frames(a['sums'], a['R'], a['first'], a['lo'], a['params'], a['B'], a['Tm'], a['H'], a['W'], a['Hc'], a['Wc'],
                                          a['out'], a['flags'], None)
    for kw in (dict(sums=None), dict(first=None), dict(out=None), dict(R=0), dict(B=0), dict(Tm=0), dict(H=0), dict(W=0), dict(Hc=0), dict(Wc=0),
               dict(sums=0x10008), dict(out=0x50004), dict(first=0x20004), dict(lo=0x30004), dict(params=0x40002), dict(flags=0x60001)):
        assert frames(**kw) == INVALID, kw
    for kw in (dict(Wc=40), dict(W=65537), dict(W=16384, Wc=4096)):           # the error returns of eas_stacked_hist_frames
        assert frames(**kw) == UNSUPPORTED, kw
        assert lib.eas_stacked_hist_frames(0x10000, 8, 0x20000, None, None, 2, 3, 10, 18, kw.get('W', 32), 32, kw.get('Wc', 48), 0x50000, None,
                                           None) == UNSUPPORTED


def test_cpu_tensors_raise():
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.stacked_hist_bin_sums(torch.zeros(3, 20, 4, 16, dtype=torch.uint8))
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.count_store_frames(torch.zeros(3, 2, 4, 16, dtype=torch.uint16), torch.zeros(2, dtype=torch.int64), 2, 32, 32)


def test_checker_equals_the_reference_fixture(golden, recordings):
    sensor, num_slice, nbins = tuple(int(v) for v in golden['sensor']), int(golden['num_slice']), int(golden['nbins'])
    assert sensor == (12, 16) and num_slice == 3 and nbins == 10 and [len(r[1]) for r in recordings] == [7, 5]
    tab = gen4_store_ref.tables(recordings, num_slice, int(golden['down_sample_factor']), sensor)
    n = len(golden['sample_names'])
    assert n == 7 and tab['sample_names'] == [str(s) for s in golden['sample_names']]
    assert [f for f, _ in tab['index']] == golden['index_file'].tolist() and [t for _, t in tab['index']] == golden['index_time'].tolist()
    assert np.array_equal(tab['boxes'], golden['raw_boxes']) and tab['boxes'].dtype == golden['raw_boxes'].dtype == np.float32
    assert np.array_equal(tab['group_start'], golden['raw_offsets'])
    # the slices: the checker's frames at the sensor's own size, and the bin sums gathered by hand
    got = gen4_store_ref.frames(recordings, tab, range(n), num_slice, *sensor)
    assert golden['slices'].shape == (n, 1, 3, 2, 12, 16) and golden['slices'].dtype == np.float64
    assert np.array_equal(got.astype(np.float64), golden['slices'])
    sums = np.concatenate([gen4_store_ref.bin_sums(r[1], nbins) for r in recordings])
    assert sums.dtype == np.uint16 and sums.shape == (12, 2, 12, 16) and sums.max() == 2550
    for i in range(n):
        for j in range(num_slice):
            k = tab['group_first'][i] + j
            want = sums[k] if k >= tab['group_lo'][i] else np.zeros((2, 12, 16))
            assert np.array_equal(golden['slices'][i, 0, j], want), (i, j)
    # what the fixture exercises: a young sequence, a sample without boxes, a box that left, boxes clipped at every border
    assert tab['group_first'][0] < 0 and not golden['slices'][0, 0, 0].any() and golden['slices'][0, 0, 1].any()
    rows = np.diff(tab['group_start']).tolist()
    assert rows == [3, 0, 2, 1, 1, 3, 1] and sum(len(r[3]) for r in recordings) == sum(rows) + 1
    b = tab['boxes']
    assert (b[:, 0] == 0).any() and (b[:, 1] == 0).any() and (b[:, 2] == 15).any() and (b[:, 3] == 11).any() and (b[:, :4] % 1 == 0.5).any()
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'gen4_store.npz')) < 64 * 1024


def assert_tables(store, tab):
    for k in TABLES:
        t = getattr(store, k)
        assert t.dtype == (torch.float32 if k == 'boxes' else torch.int64) and np.array_equal(t.numpy(), tab[k]), k
        assert np.array_equal(store.host[k], tab[k]) and store.host[k].dtype == tab[k].dtype
    assert store.sample_names == tab['sample_names'] and len(store) == len(tab['sample_names'])


def test_store_tables_names_and_order(golden, recordings):
    tab = gen4_store_ref.tables(recordings, 3, 2, (12, 16))
    store = data.Gen4Store(recordings, 3, 'cpu', sensor_hw=(12, 16), chunk=2)
    assert_tables(store, tab)
    assert store.sums is None and store.names == ['stream_a', 'stream_b'] and store.max_group_rows == 3 and store.num_slice == 3
    assert store.group_rows.tolist() == [3, 0, 2, 1, 1, 3, 1]
    for i in range(len(store)):
        raw = store.raw_labels(i)
        a, b = tab['group_start'][i], tab['group_start'][i + 1]
        box = golden['raw_boxes'][a:b]
        assert raw.dtype == np.float32 and raw.shape == (b - a, 5)
        assert np.array_equal(raw, np.stack([box[:, 0], box[:, 1], box[:, 2] - box[:, 0], box[:, 3] - box[:, 1], box[:, 4]], axis=-1))
        assert int(store.sample_names[i].split('a')[-1]) == int(recordings[tab['index'][i][0]][5][tab['index'][i][1]])
    # another num_slice and factor move the start indices, the names and the boxes; structured label rows are read as the float rows are
    lab = [np.zeros(len(r[3]), dtype=data.GEN4_BBOX_DTYPE) for r in recordings]
    for a, r in zip(lab, recordings):
        for k, name in enumerate(data.GEN4_LABEL_FIELDS):
            a[name] = r[3][:, k]
    structured = [(r[0], r[1], r[2], a, r[4], r[5]) for r, a in zip(recordings, lab)]
    assert_tables(data.Gen4Store(structured, 3, 'cpu', sensor_hw=(12, 16)), tab)
    other = data.Gen4Store(recordings, 5, 'cpu', down_sample_factor=1, sensor_hw=(12, 16))
    assert_tables(other, gen4_store_ref.tables(recordings, 5, 1, (12, 16)))
    assert other.sample_names[0] == 'stream_a_n5_a150' and other.group_first.tolist()[0] == -3 and other.group_rows.sum() == 12      # factor 1: no clip, no row leaves
    # the reference's assertion, and a shape that is not the sensor's
    name, rep, o2r, rows, o2l, times = recordings[0]
    with pytest.raises(ValueError, match='label times'):
        data.Gen4Store([(name, rep, o2r, rows, o2l, times[:-1])], 3, 'cpu', sensor_hw=(12, 16))
    with pytest.raises(ValueError, match='expected'):
        data.Gen4Store(recordings, 3, 'cpu', sensor_hw=(12, 32))


def write_tree(root, recordings):
    for name, rep, o2r, rows, o2l, times in recordings:
        label_dir, rep_dir = root / name / 'labels_v2', root / name / 'event_representations_v2' / data.GEN4_REP_NAME
        os.makedirs(label_dir)
        os.makedirs(rep_dir)
        lab = np.zeros(len(rows), dtype=data.GEN4_BBOX_DTYPE)
        for k, field in enumerate(data.GEN4_LABEL_FIELDS):
            lab[field] = rows[:, k]
        np.savez(str(label_dir / 'labels.npz'), labels=lab, objframe_idx_2_label_idx=o2l)
        np.save(str(label_dir / 'timestamps_us.npy'), times)
        np.save(str(rep_dir / 'objframe_idx_2_repr_idx.npy'), o2r)
        np.save(str(rep_dir / 'representations.npy'), rep)


def test_store_reads_directories(recordings, tmp_path):
    write_tree(tmp_path / 'train', recordings[1:])
    write_tree(tmp_path / 'val', recordings[:1])
    seen = []

    def read(rep_dir):
        seen.append(rep_dir)
        return np.load(os.path.join(rep_dir, 'representations.npy'), mmap_mode='r')
    store = data.Gen4Store.from_directories([str(tmp_path / 'train'), str(tmp_path / 'val')], 3, 'cpu', sensor_hw=(12, 16), read_representations=read)
    assert_tables(store, gen4_store_ref.tables(recordings[1:] + recordings[:1], 3, 2, (12, 16)))
    assert [os.path.basename(os.path.dirname(os.path.dirname(os.path.dirname(s)))) for s in seen] == ['train', 'val']
    one = data.Gen4Store.from_directories(str(tmp_path / 'val'), 3, 'cpu', sensor_hw=(12, 16), read_representations=read)
    assert one.sample_names == store.sample_names[3:]
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match='h5py') as err:
            data.Gen4Store.from_directories(str(tmp_path / 'val'), 3, 'cpu', sensor_hw=(12, 16))
        assert 'read_representations' in str(err.value)


def test_synthetic_recordings_are_seeded_and_varied():
    a, b, c = (data.synth_gen4_recordings(2, 12, (12, 16), 10, 3, seed=s) for s in (4, 4, 5))
    for (n1, r1, o1, l1, f1, t1), (n2, r2, o2, l2, f2, t2), (n3, r3, _, _, _, _) in zip(a, b, c):
        assert n1 == n2 != n3 and np.array_equal(r1, r2) and np.array_equal(l1, l2) and not np.array_equal(r1, r3)
        assert r1.dtype == np.uint8 and r1.shape == (12, 20, 12, 16) and r1.any() and l1.dtype == data.GEN4_BBOX_DTYPE
        assert o1.tolist() == [1, 3, 4, 6, 7, 9, 10] and len(t1) == len(o1) == len(f1) and (np.diff(t1) > 0).all()
        assert np.diff(np.r_[f1, len(l1)]).tolist() == [3, 0, 1, 2, 3, 0, 1]
        assert (l1['x'] < 0).any() or (l1['x'] + l1['w'] > 32).any() or (l1['y'] + l1['h'] > 24).any()
    store = data.Gen4Store(a, 3, 'cpu', sensor_hw=(12, 16))
    assert len(store) == 14 and store.group_first[0] == -1 and all(re.fullmatch(r'.+_n3_a\d+', n) for n in store.sample_names)


def test_loader_draws_are_a_function_of_seed_and_epoch(recordings):
    exp = types.SimpleNamespace(Tm=3, Tl=1, input_size=(32, 48), num_classes=3)
    store = data.Gen4Store(recordings, 3, 'cpu', sensor_hw=(12, 16))
    loader = data.Gen4StoreLoader(exp, 2, store=store, seed=3)
    assert len(loader) == 3 and len(loader.dataset) == 7 and loader.dataset.sample_names is store.sample_names
    a, b, other, seeded = loader.batches(0), data.Gen4StoreLoader(exp, 2, store=store, seed=3).batches(0), loader.batches(1), \
        data.Gen4StoreLoader(exp, 2, store=store, seed=4).batches(0)
    for (i1, p1, q1), (i2, p2, q2) in zip(a, b):
        assert np.array_equal(i1, i2) and np.array_equal(p1, p2) and np.array_equal(q1, q2)
        assert i1.dtype == np.int64 and p1.shape == (2, 5) and p1.dtype == np.int32 and q1.shape == (2, 3) and q1.dtype == np.int32
        for s, row in zip(i1, q1):
            n = int(store.group_rows[s])
            assert sorted(row[:n]) == list(range(n)) and list(row[n:]) == list(range(n, 3))
    assert len(set(np.concatenate([d[0] for d in a]).tolist())) == 6
    assert any(not np.array_equal(x[0], y[0]) or not np.array_equal(x[1], y[1]) for x, y in zip(a, other))
    assert any(not np.array_equal(x[0], y[0]) or not np.array_equal(x[1], y[1]) for x, y in zip(a, seeded))
    # the draws of a sample come in get_random_data's order: the six of jitter_params, then the permutation of its boxes
    rs = np.random.RandomState(3 * 1_000_003 % (1 << 32))
    order = rs.permutation(7)
    assert np.array_equal(order[:2], a[0][0])
    for b_, s in enumerate(order[:2]):
        assert tuple(a[0][1][b_]) == data.jitter_params(12, 16, 32, 48, jitter=.3, rng=rs)
        n = int(store.group_rows[s])
        assert np.array_equal(a[0][2][b_, :n], rs.permutation(n))
    exp.Tm = 4
    with pytest.raises(ValueError, match='slices per sample'):
        store.frames(torch.zeros(1, dtype=torch.int64), None, exp)


def test_experiment_selects_the_loaders(monkeypatch):
    """``train_input = 'hist_store'`` hands out the three new classes over host-side stores (no device is touched: the stores are built
    with ``device='cpu'``); ``'stacked_hist'`` still selects the synthetic loader"""
    from yolox.exp import get_exp
    e = get_exp(None, 'e-yolox-s')
    e.train_input = 'stacked_hist'
    assert type(e.get_data_loader(4, False)) is data.SyntheticStackedHistLoader
    e = get_exp(None, 'e-yolox-s')
    e.merge(['input_size', '(32, 48)', 'test_size', '(32, 48)', 'num_classes', '3'])
    e.train_input, e.store_recordings = 'hist_store', (2, 12)
    real = data.hist_store_for
    monkeypatch.setattr(data, 'hist_store_for', lambda exp, split='train', device=None: real(exp, split, 'cpu'))
    loader = e.get_data_loader(4, False)
    assert type(loader) is data.Gen4StoreLoader and len(loader) == 3 and loader.store.sensor_hw == (32, 48) and loader.store.num_slice == e.Tm
    assert e.get_data_loader(4, False).store is loader.store                    # one store per split, kept on the experiment
    ds = e.get_eval_dataset()
    assert type(ds) is data.Gen4StoreDataset and ds.store is not loader.store and len(ds) == 14 and ds.map_val and not ds.random_aug
    ev = e.get_eval_loader(2, False)
    assert type(ev) is data.Gen4StoreEvalLoader and ev.batch_size == 4 and ev.store is ds.store and len(ev) == 4
    assert ev.labels[3].dtype == torch.float32 and np.array_equal(ev.labels[3].numpy(), ds.store.raw_labels(3))
