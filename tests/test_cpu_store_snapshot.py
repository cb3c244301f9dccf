"""CPU tests of the store snapshots: the digest's definition (tests/snapshot_ref.py) against its known answers and against
``ops.bytes_digest`` on CPU tensors; the library declares, exports and binds ``eas_bytes_digest`` at ABI 9; ``save`` -> ``load_store`` of
the three stores that build on the host, whole and as a shard, read back by the independent reader as well; the errors of a damaged
file; ``exp.store_cache`` over a Gen1 dataset directory.  Everything is a copy: every comparison is exact."""
import ctypes
import os
import re
import types
import warnings

import numpy as np
import pytest
import torch

import snapshot_ref as ref
from conftest import ROOT
from eas_snn_amd import _lib, data, ops

CANVAS, TM = (64, 96), 4
SENSOR = (60, 76)


# ------------------------------------------------------------------------------------------------ the digest
def test_reference_gives_the_known_answers():
    for buf, want in zip(ref.known_inputs(), ref.KNOWN):
        assert ref.digest(buf) == want and ref.digest_slow(buf) == want
    for n in ref.LENGTHS:
        assert ref.digest(ref.random_bytes(n)) == ref.digest_slow(ref.random_bytes(n))


@pytest.mark.parametrize('n', ref.LENGTHS)
def test_bytes_digest_on_cpu_tensors_is_the_definition(n):
    buf = ref.random_bytes(n, seed=1)
    out = ops.bytes_digest(torch.from_numpy(buf))
    assert out.dtype == torch.uint64 and out.shape == (2,) and out.device.type == 'cpu'
    assert ops.bytes_digest_host(torch.from_numpy(buf)) == ref.digest(buf)
    assert tuple(int(v) for v in out.view(torch.int64).numpy().view(np.uint64)) == ref.digest(buf)


def test_bytes_digest_reads_bytes_whatever_the_dtype_and_walks_long_buffers_in_steps(monkeypatch):
    a = np.random.default_rng(3).integers(-2 ** 40, 2 ** 40, size=(7, 3, 5), dtype=np.int64)
    assert ops.bytes_digest_host(torch.from_numpy(a)) == ref.digest(a.tobytes())
    f = np.random.default_rng(4).random((11, 5)).astype(np.float32)
    assert ops.bytes_digest_host(torch.from_numpy(f)) == ref.digest(f.tobytes())
    from eas_snn_amd import ops_events
    monkeypatch.setattr(ops_events, '_DIGEST_HOST_WORDS', 64)                  # several steps, the last one partial, the word index carried on
    for buf, want in zip(ref.known_inputs(), ref.KNOWN):
        assert ops.bytes_digest_host(torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy())) == want
    with pytest.raises(AssertionError):
        ops.bytes_digest(torch.zeros(4, 4)[:, ::2])


def test_library_declares_exports_and_binds_the_digest_at_abi_9():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'eas_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+eas_bytes_digest\s*\(\s*const void\*\s*buf,\s*long long nbytes,\s*unsigned long long\*\s*out2,\s*eas_stream_t stream\)', src)
    assert _lib.PROTOTYPES['eas_bytes_digest'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p])
    lib = _lib.lib()
    assert hasattr(lib, 'eas_bytes_digest') and _lib.ABI_VERSION == 9 == lib.eas_abi_version()
    assert 'digest.hip' in open(os.path.join(ROOT, 'eas_snn_amd', 'csrc', 'Makefile')).read()
    # refused before any HIP call (no GPU here): a NULL or misaligned pointer, a negative or oversized length
    for args in ((0, 16, 8), (16, 16, 0), (8, 16, 64), (16, 16, 4), (16, -1, 64), (16, (1 << 40) + 1, 64)):
        assert lib.eas_bytes_digest(args[0], args[1], args[2], None) == -1, args


# ------------------------------------------------------------------------------------------------ round trips on the host
def exp_for(Tl=1, **kw):
    return types.SimpleNamespace(Tm=TM, Tl=Tl, input_size=CANVAS, test_size=CANVAS, num_classes=3, window=-50, aggregation='micro_sum', **kw)


def build_store(kind, shard):
    if kind == 'gen1':
        return data.Gen1Store(data.synth_gen1_recordings(3, 4, n_events=2000, sensor_hw=SENSOR), 1, (-50_000, 0), 'cpu', sensor_hw=SENSOR, shard=shard)
    if kind == 'gen4':
        return data.Gen4Store(data.synth_gen4_recordings(3, 7, sensor_hw=(24, 32)), TM, 'cpu', sensor_hw=(24, 32), shard=shard)
    return data.NCaltechStore(data.synth_ncaltech_recordings(6, 800, sensor_hw=SENSOR), 1, None, 'cpu', sensor_hw=SENSOR, shard=shard)


LOADERS = {'gen1': data.Gen1StoreLoader, 'gen4': data.Gen4StoreLoader, 'atis': data.NCaltechStoreLoader}


def same_array(a, b):
    return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def assert_same_store(got, want):
    assert type(got) is type(want) and len(got) == len(want)
    assert list(got.host) == list(want.host) and all(same_array(v, got.host[k]) for k, v in want.host.items())
    for k, v in want.host.items():
        t = getattr(got, k)
        assert t.device == got.device and np.array_equal(t.cpu().numpy(), v)
    assert getattr(got, 'names', None) == getattr(want, 'names', None) and got.sample_names == want.sample_names
    assert same_array(want.owned_samples, got.owned_samples) and got.shard == want.shard and got.sharded == want.sharded
    assert (want.sample_rank is None and got.sample_rank is None) or same_array(want.sample_rank, got.sample_rank)
    assert same_array(want.group_rows, got.group_rows) and got.max_group_rows == want.max_group_rows and got.sensor_hw == want.sensor_hw
    for k in type(want)._snapshot_fields['scalars'] + type(want)._snapshot_fields['lists']:
        assert getattr(got, k) == getattr(want, k) and type(getattr(got, k)) is type(getattr(want, k)), k
    for i in range(len(want)):
        assert same_array(want.raw_labels(i), got.raw_labels(i))
    every = np.arange(-1, len(want) + 1)
    assert np.array_equal(got.owns(every), want.owns(every))


@pytest.mark.parametrize('shard', [None, (1, 2)])
@pytest.mark.parametrize('kind', ['gen1', 'gen4', 'atis'])
def test_round_trip_on_the_host(kind, shard, tmp_path):
    want = build_store(kind, shard)
    path = str(tmp_path / 'store.eas')
    assert want.save(path) == path and os.listdir(str(tmp_path)) == ['store.eas']
    got = data.load_store(path, 'cpu', expect_shard=shard)
    assert_same_store(got, want)
    assert not hasattr(got, '_arena') and got.device == torch.device('cpu')
    if kind == 'gen4':
        assert got.sums is None and same_array(want.held_offsets, got.held_offsets) and same_array(want.group_file, got.group_file)
        assert torch.equal(got.held_first, want.held_first) and torch.equal(got.held_lo, want.held_lo)
    else:
        assert got.records.dtype == torch.uint8 and torch.equal(got.records, want.records) and want.records.numel() > 0
    exp = exp_for()
    a, b = LOADERS[kind](exp, 2, store=want, seed=3), LOADERS[kind](exp, 2, store=got, seed=3)
    assert len(a) == len(b) >= 1
    for x, y in zip(a.batches(0), b.batches(0)):
        assert len(x) == len(y) and all(same_array(u, v) for u, v in zip(x, y))
    with pytest.raises(data.SnapshotError, match='shard'):
        data.load_store(path, 'cpu', expect_shard=(0, 2))
    # the independent reader: the layout and the digests as the header states them, and the same bytes
    header, arrays = ref.read_snapshot(path)
    assert header['class'] == type(want).__name__ and header['key'] is None and header['shard'] == (None if shard is None else list(shard))
    assert header['sample_names'] == want.sample_names
    for k, v in want.host.items():
        assert same_array(v, arrays[k])
    places = {e['name']: e['where'] for e in header['sections']}
    assert all(places[k] == 'host' for k in want.host) and places['sample_file'] == 'host'
    if kind != 'gen4':
        assert places['records'] == 'device' and np.array_equal(arrays['records'], want.records.numpy())
    for k in ('Tl', 'window', 'sensor_hw', 'num_slice', 'nbins', 'down_sample_factor', 'max_file_records'):
        if hasattr(want, k):
            v = getattr(want, k)
            assert header['scalars'][k] == (list(v) if isinstance(v, tuple) else v), k


# ------------------------------------------------------------------------------------------------ errors
@pytest.fixture()
def saved(tmp_path):
    store = build_store('gen1', None)
    path = str(tmp_path / 'store.eas')
    store.save(path)
    return store, path, ref.read_snapshot(path)[0]


def rewrite(path, edit):
    raw = bytearray(open(path, 'rb').read())
    raw = edit(raw)
    with open(path, 'wb') as f:
        f.write(bytes(raw))


@pytest.mark.parametrize('section', ['records', 'boxes', 'group_t'])
def test_a_flipped_byte_names_the_file_and_the_section(saved, section):
    _, path, header = saved
    e = next(e for e in header['sections'] if e['name'] == section)
    assert e['nbytes'] > 0

    def flip(raw):
        raw[e['offset'] + e['nbytes'] // 2] ^= 0x10
        return raw
    rewrite(path, flip)
    with pytest.raises(data.SnapshotError, match=re.escape(path) + '.*' + repr(section)) as err:
        data.load_store(path, 'cpu')
    assert isinstance(err.value, ValueError) and 'digest' in str(err.value)


def test_a_short_file_a_wrong_magic_and_a_later_version_are_refused(saved):
    _, path, header = saved
    good = open(path, 'rb').read()
    last = [e for e in header['sections'] if e['nbytes']][-1]
    assert last['offset'] + last['nbytes'] == len(good)                      # nothing behind the last section: one byte less cuts into it
    rewrite(path, lambda raw: raw[:-1])
    with pytest.raises(data.SnapshotError, match=re.escape(path) + '.*' + repr(last['name'])):
        data.load_store(path, 'cpu')
    rewrite(path, lambda raw: bytearray(b'EASSTORF') + bytearray(good[8:]))
    with pytest.raises(data.SnapshotError, match=re.escape(path) + '.*magic'):
        data.load_store(path, 'cpu')
    rewrite(path, lambda raw: bytearray(good[:8]) + bytearray((ref.VERSION + 1).to_bytes(4, 'little')) + bytearray(good[12:]))
    with pytest.raises(data.SnapshotError, match=re.escape(path) + '.*version 2'):
        data.load_store(path, 'cpu')
    rewrite(path, lambda raw: bytearray(good[:40]))                            # cut inside the header
    with pytest.raises(data.SnapshotError, match=re.escape(path)):
        data.load_store(path, 'cpu')
    rewrite(path, lambda raw: bytearray(good))
    assert_same_store(data.load_store(path, 'cpu'), saved[0])


def test_a_byte_length_that_does_not_match_is_refused(saved):
    import json
    _, path, header = saved
    good = open(path, 'rb').read()
    length = int.from_bytes(good[12:20], 'little')
    e = next(e for e in header['sections'] if e['name'] == 'group_t')
    e['nbytes'] -= 8
    blob = json.dumps(header).encode()
    assert len(blob) <= length
    rewrite(path, lambda raw: bytearray(good[:12]) + bytearray(len(blob).to_bytes(8, 'little')) + bytearray(blob) + bytearray(good[20 + len(blob):]))
    with pytest.raises(data.SnapshotError, match=re.escape(path) + ".*'group_t'"):
        data.load_store(path, 'cpu')


def test_a_tmp_file_left_behind_is_ignored_and_overwritten(saved, tmp_path):
    store, path, _ = saved
    other = str(tmp_path / 'other.eas')
    with open(other + '.tmp', 'wb') as f:
        f.write(b'half a snapshot')
    assert not os.path.exists(other)
    with pytest.raises(FileNotFoundError):
        data.load_store(other, 'cpu')
    store.save(other)
    assert not os.path.exists(other + '.tmp') and open(other, 'rb').read() == open(path, 'rb').read()
    assert_same_store(data.load_store(other, 'cpu'), store)


# ------------------------------------------------------------------------------------------------ exp.store_cache
@pytest.fixture()
def dataset(tmp_path):
    root = tmp_path / 'gen1'
    recs = data.synth_gen1_recordings(4, 4, n_events=2000, sensor_hw=SENSOR)
    for d, part in (('train', recs[:3]), ('val', recs[3:])):
        os.makedirs(str(root / d))
        for name, dat, rows in part:
            dat.tofile(str(root / d / f'{name}_td.dat'))
            np.save(str(root / d / f'{name}_bbox.npy'), rows)
    return str(root), str(tmp_path / 'cache')


def cache_exp(dataset, **kw):
    root, cache = dataset
    kw.setdefault('store_cache', cache)
    return exp_for(data_dir=root, **kw)


def eas_files(cache):
    return sorted(os.listdir(cache)) if os.path.isdir(cache) else []


def test_store_cache_builds_once_then_loads(dataset, monkeypatch):
    root, cache = dataset
    built = data.gen1_store_for(cache_exp(dataset), device='cpu')
    assert type(built) is data.Gen1Store and len(built) == 16 and hasattr(built, '_owner_args')
    files = eas_files(cache)
    assert len(files) == 1 and re.fullmatch(r'dat_store_train_[0-9a-f]{16}\.eas', files[0])
    header, _ = ref.read_snapshot(os.path.join(cache, files[0]))
    key = header['key']
    assert key['format'] == ref.VERSION and key['cls'] == 'Gen1Store' and key['shard'] is None and key['args']['Tl'] == 1
    assert sorted(s[0] for s in key['sources']) == sorted(os.path.join(d, f) for d in ('train', 'val') for f in os.listdir(os.path.join(root, d)))
    for rel, size, mtime in key['sources']:
        st = os.stat(os.path.join(root, rel))
        assert (size, mtime) == (st.st_size, st.st_mtime_ns)
    before = os.stat(os.path.join(cache, files[0])).st_mtime_ns

    def refuse(*a, **k):
        raise AssertionError('the store was built although its snapshot is current')
    monkeypatch.setattr(data.Gen1Store, 'from_directories', classmethod(refuse))
    exp = cache_exp(dataset)
    loaded = data.gen1_store_for(exp, device='cpu')
    assert loaded is not built and data.gen1_store_for(exp, device='cpu') is loaded
    assert_same_store(loaded, built)
    assert torch.equal(loaded.records, built.records)
    assert eas_files(cache) == files and os.stat(os.path.join(cache, files[0])).st_mtime_ns == before


def test_store_cache_rebuilds_when_a_source_or_an_argument_changes(dataset):
    root, cache = dataset
    data.gen1_store_for(cache_exp(dataset), device='cpu')
    first = eas_files(cache)
    dat = os.path.join(root, 'train', sorted(f for f in os.listdir(os.path.join(root, 'train')) if f.endswith('_td.dat'))[0])
    st = os.stat(dat)
    os.utime(dat, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    data.gen1_store_for(cache_exp(dataset), device='cpu')
    second = eas_files(cache)
    assert len(second) == 2 and set(first) < set(second)
    other_tl = data.gen1_store_for(cache_exp(dataset, Tl=2), device='cpu')
    third = eas_files(cache)
    assert len(third) == 3 and set(second) < set(third) and other_tl.Tl == 2
    name = os.path.basename(dat)[:-len('_td.dat')]
    fewer = data.gen1_store_for(cache_exp(dataset, store_ignore=(name,)), device='cpu')
    assert len(eas_files(cache)) == 4 and name not in fewer.names and len(fewer.names) == 3
    again = data.gen1_store_for(cache_exp(dataset, store_ignore=(name,)), device='cpu')
    assert len(eas_files(cache)) == 4 and not hasattr(again, '_arena')
    assert_same_store(again, fewer)


def test_store_cache_warns_once_about_a_corrupted_file_and_writes_it_again(dataset):
    root, cache = dataset
    built = data.gen1_store_for(cache_exp(dataset), device='cpu')
    (name,) = eas_files(cache)
    path = os.path.join(cache, name)
    good = open(path, 'rb').read()
    e = next(e for e in ref.read_snapshot(path)[0]['sections'] if e['name'] == 'records')
    rewrite(path, lambda raw: raw[:e['offset'] + 5] + bytearray([raw[e['offset'] + 5] ^ 1]) + raw[e['offset'] + 6:])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        rebuilt = data.gen1_store_for(cache_exp(dataset), device='cpu')
    assert len(caught) == 1 and path in str(caught[0].message) and "'records'" in str(caught[0].message)
    assert_same_store(rebuilt, built)
    assert eas_files(cache) == [name] and open(path, 'rb').read() == good
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert_same_store(data.gen1_store_for(cache_exp(dataset), device='cpu'), built)


def test_without_store_cache_nothing_is_written(dataset):
    root, cache = dataset
    from yolox.exp import get_exp
    assert get_exp(None, 'e-yolox-s').store_cache is None
    store = data.gen1_store_for(cache_exp(dataset, store_cache=None), device='cpu')
    assert len(store) == 16 and not os.path.exists(cache)
    assert sorted(os.listdir(os.path.dirname(cache))) == ['gen1']
    # a synthetic store (no dataset directory) is never cached
    data.gen1_store_for(exp_for(data_dir=os.path.join(root, 'missing'), store_cache=cache, store_recordings=(2, 4, 1000)), device='cpu')
    assert not os.path.exists(cache)


def test_store_cache_keeps_one_file_per_rank_of_a_sharded_store(dataset, monkeypatch):
    import yolox.utils
    root, cache = dataset
    monkeypatch.setattr(yolox.utils, 'get_world_size', lambda: 2)
    built = {}
    for rank in (0, 1):
        monkeypatch.setattr(yolox.utils, 'get_rank', lambda: rank)
        built[rank] = data.gen1_store_for(cache_exp(dataset, store_shard='recordings'), device='cpu')
    files = sorted(eas_files(cache), key=lambda f: f[-len('_r0of2.eas'):])       # (the keys differ with the sources: by rank, not by name)
    assert len(files) == 2 and files[0].endswith('_r0of2.eas') and files[1].endswith('_r1of2.eas')
    assert built[0].records.numel() > 0 and built[1].records.numel() > 0
    assert sorted(np.concatenate([built[0].owned_samples, built[1].owned_samples]).tolist()) == list(range(16))
    monkeypatch.setattr(data.Gen1Store, 'from_directories', classmethod(lambda *a, **k: 1 / 0))
    for rank in (0, 1):
        monkeypatch.setattr(yolox.utils, 'get_rank', lambda: rank)
        loaded = data.gen1_store_for(cache_exp(dataset, store_shard='recordings'), device='cpu')
        assert loaded.shard == (rank, 2) and torch.equal(loaded.records, built[rank].records)
        assert_same_store(loaded, built[rank])
        # a rank's file holds the .dat files of its own recordings only
        header, _ = ref.read_snapshot(os.path.join(cache, files[rank]))
        dats = {os.path.basename(s[0])[:-len('_td.dat')] for s in header['key']['sources'] if s[0].endswith('_td.dat')}
        assert dats == {n for n, r in loaded._owner_ranks.items() if r == rank}
    assert sorted(eas_files(cache)) == sorted(files)


def test_replica_mode_only_rank_0_writes(dataset, monkeypatch):
    import yolox.utils
    root, cache = dataset
    monkeypatch.setattr(yolox.utils, 'get_world_size', lambda: 2)
    monkeypatch.setattr(yolox.utils, 'get_rank', lambda: 1)
    other = data.gen1_store_for(cache_exp(dataset), device='cpu')                # no file yet: rank 1 builds and does not wait or write
    assert eas_files(cache) == [] and hasattr(other, '_owner_args')
    monkeypatch.setattr(yolox.utils, 'get_rank', lambda: 0)
    data.gen1_store_for(cache_exp(dataset), device='cpu')
    (name,) = eas_files(cache)
    assert '_r' not in name[len('dat_store_train_'):]
    monkeypatch.setattr(yolox.utils, 'get_rank', lambda: 1)
    monkeypatch.setattr(data.Gen1Store, 'from_directories', classmethod(lambda *a, **k: 1 / 0))
    assert_same_store(data.gen1_store_for(cache_exp(dataset), device='cpu'), other)


def test_store_cache_of_the_other_two_inputs(tmp_path, monkeypatch):
    """N-Caltech101 (the split file is the listing) and 1 Mpx (the representations through a reader of the test's own): built once, then
    loaded; a touched source file gives another key"""
    cache = str(tmp_path / 'cache')
    atis = tmp_path / 'ncaltech'
    lines = []
    for c, stem, rec, ann in data.synth_ncaltech_recordings(6, 800, sensor_hw=SENSOR):
        os.makedirs(str(atis / 'Caltech101' / c), exist_ok=True)
        os.makedirs(str(atis / 'Caltech101_annotations' / c), exist_ok=True)
        rec.tofile(str(atis / 'Caltech101' / c / f'{stem}.bin'))
        ann.tofile(str(atis / 'Caltech101_annotations' / c / f'annotation_{stem}.bin'))
        lines.append(f'Caltech101/{c}/{stem}.bin Caltech101_annotations/{c}/annotation_{stem}.bin\n')
    with open(str(atis / 'train.txt'), 'w') as f:
        f.writelines(lines)
    built = data.ncaltech_store_for(exp_for(data_dir=str(atis), store_cache=cache), device='cpu')
    (name,) = eas_files(cache)
    assert name.startswith('atis_store_train_') and len(built) == 6
    key = ref.read_snapshot(os.path.join(cache, name))[0]['key']
    assert len(key['sources']) == 1 + 2 * 6 and key['args']['class_names'] == built.class_names
    with monkeypatch.context() as m:
        m.setattr(data.NCaltechStore, 'from_directory', classmethod(lambda *a, **k: 1 / 0))
        assert_same_store(data.ncaltech_store_for(exp_for(data_dir=str(atis), store_cache=cache), device='cpu'), built)
    st = os.stat(str(atis / 'train.txt'))
    os.utime(str(atis / 'train.txt'), ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    data.ncaltech_store_for(exp_for(data_dir=str(atis), store_cache=cache), device='cpu')
    assert len(eas_files(cache)) == 2

    gen4 = tmp_path / 'gen4'
    for d, part in (('train', data.synth_gen4_recordings(2, 3, seed=0)), ('val', data.synth_gen4_recordings(1, 3, seed=1))):   # (the factory's sensor: 360 x 640)
        for stream, reps, obj2repr, rows, obj2label, times in part:
            label_dir, rep_dir = gen4 / d / stream / 'labels_v2', gen4 / d / stream / 'event_representations_v2' / data.GEN4_REP_NAME
            os.makedirs(str(label_dir))
            os.makedirs(str(rep_dir))
            np.savez(str(label_dir / 'labels.npz'), labels=rows, objframe_idx_2_label_idx=obj2label)
            np.save(str(label_dir / 'timestamps_us.npy'), times)
            np.save(str(rep_dir / 'objframe_idx_2_repr_idx.npy'), obj2repr)
            np.save(str(rep_dir / 'representations.npy'), reps)
    monkeypatch.setattr(data, '_h5_representations', lambda rep_dir: np.load(os.path.join(rep_dir, 'representations.npy'), mmap_mode='r'))
    hist = data.hist_store_for(exp_for(data_dir=str(gen4), store_cache=cache), device='cpu')
    names = [n for n in eas_files(cache) if n.startswith('hist_store_train_')]
    assert len(names) == 1 and len(hist.names) == 3
    key = ref.read_snapshot(os.path.join(cache, names[0]))[0]['key']
    assert len(key['sources']) == 3 * 4 and key['args']['store_sums'] == 'u16' and key['cls'] == 'Gen4Store'
    with monkeypatch.context() as m:
        m.setattr(data.Gen4Store, 'from_directories', classmethod(lambda *a, **k: 1 / 0))
        assert_same_store(data.hist_store_for(exp_for(data_dir=str(gen4), store_cache=cache), device='cpu'), hist)
    data.hist_store_for(exp_for(data_dir=str(gen4), store_cache=cache, store_sums='packed'), device='cpu')
    assert len([n for n in eas_files(cache) if n.startswith('hist_store_train_')]) == 2
