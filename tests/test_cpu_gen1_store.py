"""CPU-only tests of Gen1 training from recordings in HBM: the numpy checker of the label kernel (tests/labels_ref.py) equals
tests/golden/gen1_labels.npz -- recorded from the reference's own ``get_random_data`` / ``reformat`` / ``TrainTransform``
(scripts/gen_golden_gen1_labels.py) -- bit for bit, ``jitter_params`` / ``letterbox_params`` reproduce its resize sizes from its draws;
``eas_label_targets`` is declared, exported, bound and refuses bad arguments before any launch; ``data.parse_dat_header`` equals the
oracle's; the tables, names and sample order of ``data.Gen1Store`` on host tensors; the draws of ``data.Gen1StoreLoader``."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import labels_ref
import eas_snn_amd
from eas_snn_amd import data, ops
from oracle import events_ref

INVALID = -1


def fixture_cases():
    return labels_ref.fixture_cases(load_golden('gen1_labels'))


case_params = labels_ref.case_params


def test_checker_equals_the_reference_fixture():
    seen = {}
    for name, case in fixture_cases():
        (ih, iw), (h, w) = case['sensor'], case['canvas']
        par = case_params(case)
        assert tuple(par[:2]) == case['dsize'], name                           # the size the reference asked its resize for
        t, count, flags, box = labels_ref.sample_targets(case['raw'], par, ih, iw, h, w, perm_row=case['perm'])
        assert flags == 0 and count == len(case['rows']), name
        assert box.dtype == case['boxes'].dtype == np.float32 and np.array_equal(box, case['boxes']), name
        assert t.dtype == case['targets'].dtype == np.float32 and np.array_equal(t, case['targets']), name
        # the survivors are the rows the reference kept, in the order of the permutation
        assert [int(r) for r in case['perm'] if r in set(case['rows'].tolist())] == case['rows'].tolist(), name
        seen[name] = (len(case['raw']), count, par[4])
    assert len(seen) == 48 and {n.split('_')[0] for n in seen} == {'gen1', 'small'}
    for geo in ('gen1', 'small'):
        assert seen[f'{geo}_none_flip'][:2] == (0, 0) and seen[f'{geo}_one_letterbox'][:2] == (1, 1)
        assert seen[f'{geo}_many_flip'][:2] == (70, 70) and seen[f'{geo}_many_noflip'][:2] == (70, 70)        # the cut at 50 is exercised
        assert seen[f'{geo}_tiny_flip'][1] < 6 and seen[f'{geo}_tiny_resize'][1] < 6                          # boxes of at most 1 px leave
        assert seen[f'{geo}_borders_flip'][2] == 1 and seen[f'{geo}_borders_noflip'][2] == 0
    cases = dict(fixture_cases())
    assert (cases['gen1_negative_flip']['raw'][:, :4] < 0).any() and (cases['gen1_negative_flip']['raw'][:, :4] % 1 != 0).any()
    assert cases['gen1_many_flip']['targets'][49].any() and cases['gen1_one_flip']['sensor'] == (240, 304)
    assert cases['gen1_one_flip']['canvas'] == (256, 320) and cases['small_one_flip']['sensor'] == (36, 48) and cases['small_one_flip']['canvas'] == (64, 64)
    assert any((c['targets'][:, 1:3] % 1 == 0.5).any() for c in cases.values())                                # centres at halves
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'gen1_labels.npz')) < 64 * 1024


def test_truncation_toward_zero_is_what_the_fixture_pins():
    """a checker that floors the rows instead of truncating them misses the negative-corner cases: the fixture tells the two apart"""
    differ = 0
    for name, case in fixture_cases():
        if '_negative_' not in name:
            continue
        (ih, iw), (h, w) = case['sensor'], case['canvas']
        floored = np.floor(case['raw'])
        t, _, _, _ = labels_ref.sample_targets(floored, case_params(case), ih, iw, h, w, perm_row=case['perm'])
        differ += not np.array_equal(t, case['targets'])
    assert differ > 0


def test_checker_flag_rules_and_batches():
    boxes = np.array([[10, 10, 100, 100, 1], [20, 30, 90, 120, 0], [5, 5, 60, 70, 1]], dtype=np.float32)
    gs = np.array([0, 0, 3], dtype=np.int64)
    par = np.array([[304, 240, 0, 0, 0]] * 5, dtype=np.int32)
    perm = np.array([[0, 1, 2], [2, 0, 1], [2, 7, -1], [0, 1, 2], [1, 0, 2]], dtype=np.int32)
    t, count, flags = labels_ref.targets(boxes, gs, [0, 1, 1, 2, -1], par, 240, 304, 256, 320, perm=perm)
    assert list(count) == [0, 3, 1, 0, 0] and list(flags) == [0, 0, 1, 4, 4]
    assert not t[0].any() and not t[3].any() and list(t[1, :3, 0]) == [1, 1, 0] and list(t[2, 0]) == [1, 32.5, 37.5, 55, 65] and not t[2, 1:].any()
    t2, count2, flags2 = labels_ref.targets(boxes, gs, [1], par[:1], 240, 304, 256, 320, perm=perm[:1, :2], max_labels=1)
    assert list(count2) == [2] and list(flags2) == [2] and t2.shape == (1, 1, 5) and list(t2[0, 0]) == [1, 55, 55, 90, 90]
    t3, _, flags3 = labels_ref.targets(boxes, gs, [1], par[:1], 240, 304, 256, 320)
    assert flags3[0] == 0 and np.array_equal(t3[0, :3], t[1, [1, 2, 0]])       # identity order


@pytest.mark.parametrize('n', [1, 2, 3, 7, 64, 70])
def test_permutation_is_the_shuffle_of_the_rows(n):
    """``RandomState.permutation(n)`` is the order ``np.random.shuffle`` gives n rows under the same state (what the loader relies on)"""
    for seed in range(5):
        rows = np.arange(n * 5).reshape(n, 5)
        np.random.seed(seed)
        np.random.shuffle(rows)
        assert np.array_equal(rows[:, 0] // 5, np.random.RandomState(seed).permutation(n))


def test_entry_point_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    eas_snn_amd._lib._bind_host_hip_runtime()
    handle = ctypes.CDLL(eas_snn_amd._lib.LIB_PATH)
    n = 'eas_label_targets'
    assert n in declared and hasattr(handle, n) and n in eas_snn_amd._lib.PROTOTYPES
    assert sorted(eas_snn_amd._lib.PROTOTYPES) == sorted(declared)
    assert eas_snn_amd._lib.ABI_VERSION == 9 and eas_snn_amd.hip_library().eas_abi_version() == 9          # purely additive
    assert hasattr(ops, 'label_targets')
    for name in ('parse_dat_header', 'Gen1Store', 'synth_gen1_recordings', 'Gen1StoreLoader', 'Gen1StoreEvalLoader'):
        assert hasattr(data, name)
    assert data.FRAME_AGGREGATIONS == ('micro_sum', 'timesurface') and data.ATIS_MEASURES == ('count', 'timesurface')


def test_bad_arguments_are_refused_before_any_launch():
    """every call below returns from the argument checks: no device is touched (the pointers are made-up addresses)"""
    fn = eas_snn_amd.hip_library().eas_label_targets
    good = dict(boxes=0x10000, L=9, group_start=0x20000, G=3, group=0x30000, params=0x40000, perm=0x50000, P=4, B=2, ih=240, iw=304, h=256, w=320,
                max_labels=50, targets=0x60000, count=0x70000, flags=0x80000)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a['boxes'], a['L'], a['group_start'], a['G'], a['group'], a['params'], a['perm'], a['P'], a['B'], a['ih'], a['iw'], a['h'], a['w'],
                  a['max_labels'], a['targets'], a['count'], a['flags'], None)
    for kw in (dict(boxes=None), dict(group_start=None), dict(group=None), dict(params=None), dict(targets=None),
               dict(max_labels=0), dict(max_labels=-1), dict(iw=0), dict(ih=0), dict(iw=-304), dict(B=-1), dict(G=-1), dict(P=-1), dict(L=-1),
               dict(boxes=0x10002), dict(group_start=0x20004), dict(group=0x30004), dict(params=0x40001), dict(perm=0x50002), dict(targets=0x60002),
               dict(count=0x70001), dict(flags=0x80003)):
        assert call(**kw) == INVALID, kw
    assert call(B=0) == 0 and call(B=0, perm=None, P=0, count=None, flags=None) == 0        # an empty batch is no work
    assert call(B=0, max_labels=0) == INVALID                                                # bad arguments first


def test_cpu_tensors_raise():
    z = torch.zeros
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.label_targets(z(3, 5), z(2, dtype=torch.int64), z(1, dtype=torch.int64), z(1, 5, dtype=torch.int32), 240, 304, 256, 320)


def test_parse_dat_header_equals_the_oracle():
    rng = np.random.default_rng(3)
    t = np.sort(rng.integers(0, 10_000, 50))
    x, y, p = rng.integers(0, 304, 50), rng.integers(0, 240, 50), rng.integers(0, 2, 50)
    for hw in ((240, 304), (36, 48)):
        image = events_ref.encode_dat_file(t, x, y, p, *hw)
        assert data.parse_dat_header(image) == events_ref.parse_dat_header(image)
        assert data.parse_dat_header(np.frombuffer(image, dtype=np.uint8)) == events_ref.parse_dat_header(image)
        assert data.encode_dat(t, x, y, p, *hw).tobytes() == image
        start, ev_type, ev_size = data.parse_dat_header(image)
        assert (ev_type, ev_size) == (0, 8) and len(image) - start == 8 * 50
    bare = events_ref.encode_dat_file(t, x, y, p)[events_ref.parse_dat_header(events_ref.encode_dat_file(t, x, y, p))[0]:]
    assert data.parse_dat_header(bare) == events_ref.parse_dat_header(bare) == (0, 0, 8)                   # no header lines: records from byte 0
    odd = b'% one line\n' + bytes([12, 16]) + bytes(32)
    assert data.parse_dat_header(odd) == events_ref.parse_dat_header(odd) == (13, 12, 16)


@pytest.fixture(scope='module')
def recordings():
    return data.synth_gen1_recordings(3, 6, n_events=500, sensor_hw=(24, 32), seed=4)


def test_synthetic_recordings_are_seeded_and_varied(recordings):
    again = data.synth_gen1_recordings(3, 6, n_events=500, sensor_hw=(24, 32), seed=4)
    other = data.synth_gen1_recordings(3, 6, n_events=500, sensor_hw=(24, 32), seed=5)
    for (n1, d1, r1), (n2, d2, r2), (n3, d3, r3) in zip(recordings, again, other):
        assert n1 == n2 != n3 and np.array_equal(d1, d2) and np.array_equal(r1, r2) and not np.array_equal(d1, d3)
        assert d1.dtype == np.uint8 and r1.dtype.names[:6] == ('t', 'x', 'y', 'w', 'h', 'class_id')
        per_time = np.unique(r1['t'], return_counts=True)[1]
        assert list(per_time) == [3, 2, 1, 2, 3, 2]                            # several boxes at some times


def test_store_tables_names_and_order(recordings):
    store = data.Gen1Store(recordings, Tl=2, window=(-20_000, 0), device='cpu', sensor_hw=(24, 32))
    assert len(store) == 18 and store.max_group_rows == 3 and store.records.dtype == torch.uint8 and store.records.numel() == 3 * 500 * 8
    assert store.file_offsets.tolist() == [0, 500, 1000, 1500] and store.file_offsets.dtype == torch.int64
    assert store.group_start.dtype == torch.int64 and store.group_t.dtype == torch.int64 and store.group_file.dtype == torch.int32
    assert store.boxes.dtype == torch.float32 and store.boxes.shape == (3 * 13, 5)
    assert store.group_start.tolist() == list(np.cumsum([0] + [3, 2, 1, 2, 3, 2] * 3))
    assert store.group_file.tolist() == [0] * 6 + [1] * 6 + [2] * 6
    # the flat index is resolve_index's: recordings in order, groups in time order; names follow get_sample_resp
    end_idx = np.cumsum([6, 6, 6])
    for i, name in enumerate(store.sample_names):
        f = int(np.searchsorted(end_idx, i, side='right'))
        k = i - (end_idx[f - 1] if f else 0)
        rows = recordings[f][2]
        times = np.unique(rows['t'])
        assert name == f'{recordings[f][0]}_r{k}_a{int(times[k])}' and re.fullmatch(r'.+_r\d+_a\d+', name)
        assert int(store.group_t[i]) == int(times[k]) and int(name.split('a')[-1]) == int(times[k])
        mine = rows[rows['t'] == times[k]]
        a, b = int(store.group_start[i]), int(store.group_start[i + 1])
        want = np.stack([mine['x'], mine['y'], mine['x'] + mine['w'], mine['y'] + mine['h'], mine['class_id']], axis=-1)
        assert np.array_equal(store.boxes[a:b].numpy(), want.astype(np.float32))
        raw = store.raw_labels(i)
        assert raw.dtype == np.float32 and np.array_equal(raw[:, :2], want[:, :2]) and np.array_equal(raw[:, 2], want[:, 2] - want[:, 0])
    # the record areas are the files without their headers
    start = data.parse_dat_header(recordings[1][1])[0]
    assert np.array_equal(store.records[500 * 8:1000 * 8].numpy(), recordings[1][1][start:])
    # 'ts' instead of 't', names left out
    renamed = [(n, d, r.astype(np.dtype([('ts' if k == 't' else k, r.dtype[k]) for k in r.dtype.names]))) for n, d, r in recordings]
    s2 = data.Gen1Store(renamed, 2, (-20_000, 0), 'cpu', ignore=(recordings[1][0],), sensor_hw=(24, 32))
    assert len(s2) == 12 and s2.names == [recordings[0][0], recordings[2][0]] and s2.group_t.tolist() == store.group_t[[*range(6), *range(12, 18)]].tolist()


def test_store_refuses_descending_label_times(recordings):
    name, dat, rows = recordings[0]
    bad = rows.copy()
    bad['t'][4] = bad['t'][0] - 1
    with pytest.raises(ValueError):
        data.Gen1Store([(name, dat, bad)], 1, (-20_000, 0), 'cpu')
    with pytest.raises(ValueError):
        data.Gen1Store([(name, dat[:-3], rows)], 1, (-20_000, 0), 'cpu')       # not a whole number of records


def test_store_reads_directories(recordings, tmp_path):
    for sub, recs in (('train', recordings[:2]), ('val', recordings[2:])):
        os.makedirs(tmp_path / sub)
        for name, dat, rows in recs:
            dat.tofile(str(tmp_path / sub / f'{name}_td.dat'))
            np.save(str(tmp_path / sub / f'{name}_bbox.npy'), rows)
    a = data.Gen1Store.from_directories([str(tmp_path / 'train'), str(tmp_path / 'val')], 1, (-20_000, 0), 'cpu', sensor_hw=(24, 32))
    b = data.Gen1Store(recordings, 1, (-20_000, 0), 'cpu', sensor_hw=(24, 32))
    assert a.sample_names == b.sample_names and torch.equal(a.records, b.records) and torch.equal(a.boxes, b.boxes)
    assert torch.equal(a.group_start, b.group_start) and torch.equal(a.file_offsets, b.file_offsets)


def test_loader_draws_are_a_function_of_seed_and_epoch(recordings):
    exp = types.SimpleNamespace(Tm=3, Tl=1, input_size=(32, 48), num_classes=2, window=-20)
    store = data.Gen1Store(recordings, 1, (-20_000, 0), 'cpu', sensor_hw=(24, 32))
    loader = data.Gen1StoreLoader(exp, 4, store=store, seed=3)
    assert len(loader) == 4 and len(loader.dataset) == 18 and loader.dataset.sample_names is store.sample_names
    a, b, other, seeded = loader.batches(0), data.Gen1StoreLoader(exp, 4, store=store, seed=3).batches(0), loader.batches(1), \
        data.Gen1StoreLoader(exp, 4, store=store, seed=4).batches(0)
    for (i1, p1, q1), (i2, p2, q2) in zip(a, b):
        assert np.array_equal(i1, i2) and np.array_equal(p1, p2) and np.array_equal(q1, q2)
        assert i1.dtype == np.int64 and p1.shape == (4, 5) and p1.dtype == np.int32 and q1.shape == (4, 3) and q1.dtype == np.int32
        for s, row in zip(i1, q1):
            n = int(store.group_rows[s])
            assert sorted(row[:n]) == list(range(n)) and list(row[n:]) == list(range(n, 3))
    seen = np.concatenate([d[0] for d in a])
    assert len(set(seen.tolist())) == 16 and seen.min() >= 0 and seen.max() < 18                      # part of a permutation
    assert any(not np.array_equal(x[0], y[0]) or not np.array_equal(x[1], y[1]) for x, y in zip(a, other))
    assert any(not np.array_equal(x[0], y[0]) or not np.array_equal(x[1], y[1]) for x, y in zip(a, seeded))
    # the draws of a sample come in the reference's order: the six of jitter_params, then the permutation of its boxes
    rs = np.random.RandomState(3 * 1_000_003 % (1 << 32))
    order = rs.permutation(18)
    assert np.array_equal(order[:4], a[0][0])
    for b_, s in enumerate(order[:4]):
        assert tuple(a[0][1][b_]) == data.jitter_params(24, 32, 32, 48, jitter=.3, rng=rs)
        n = int(store.group_rows[s])
        assert np.array_equal(a[0][2][b_, :n], rs.permutation(n))
