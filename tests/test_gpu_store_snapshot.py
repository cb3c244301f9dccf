"""GPU tests of the store snapshots.  ``eas_bytes_digest`` against the numpy statement of its definition (tests/snapshot_ref.py) at the
smallest lengths at which the tail word, the 16-byte pairing, a single block and the grid-stride wrap can each go wrong; ``save`` ->
``load_store`` of the five stores that live on the device, whole, untrimmed and as a shard, through one chunk and through chunks of 4096
bytes; ``exp.store_cache`` up to the loader's first batch.  Everything is a copy or integer arithmetic: every comparison is exact."""
import os
import types

import numpy as np
import pytest
import torch

import snapshot_ref as ref
from eas_snn_amd import _lib, data, ops

pytestmark = pytest.mark.gpu

CANVAS, TM = (64, 96), 4
SENSOR = (60, 76)
LENGTHS = ref.LENGTHS + [(64 << 10) + 3, (8 << 20) + 5]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ the digest
@pytest.mark.parametrize('n', LENGTHS)
def test_digest_equals_the_definition(dev, n):
    buf = ref.random_bytes(n, seed=2)
    t = torch.from_numpy(buf).to(dev)
    out = ops.bytes_digest(t)
    assert out.dtype == torch.uint64 and out.shape == (2,) and out.device == t.device
    want = ref.digest(buf)
    print(f'n = {n}: got {[hex(v) for v in ops.bytes_digest_host(t)]}, want {[hex(v) for v in want]}')
    assert ops.bytes_digest_host(t) == want
    assert torch.equal(ops.bytes_digest(t).view(torch.int64), out.view(torch.int64))          # two calls: the same words


def test_digest_of_views_and_of_other_dtypes(dev):
    buf = ref.random_bytes(70_000, seed=3)
    t = torch.from_numpy(buf).to(dev)
    for a, n in ((16, 4097), (4096, 65_536 + 3), (48, 0), (32, 9)):             # 16-byte-aligned offsets into a larger buffer
        assert t[a:a + n].data_ptr() % 16 == 0 and ops.bytes_digest_host(t[a:a + n]) == ref.digest(buf[a:a + n])
    for a, n in ((1, 4097), (8, 33), (23, 1)):                                  # not aligned: the wrapper clones the view
        assert t[a:a + n].data_ptr() % 16 != 0 and ops.bytes_digest_host(t[a:a + n]) == ref.digest(buf[a:a + n])
    lib = _lib.lib()
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    assert lib.eas_bytes_digest(t[8:].data_ptr(), 64, out.data_ptr(), ops.stream()) == -1      # the entry itself refuses it
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0]
    w = np.random.default_rng(5).integers(0, 2 ** 16, size=(3, 2, 5, 7), dtype=np.uint16)
    assert ops.bytes_digest_host(torch.from_numpy(w).to(dev)) == ref.digest(w.tobytes())
    q = np.random.default_rng(6).integers(-2 ** 62, 2 ** 62, size=(9, 2), dtype=np.int64)
    assert ops.bytes_digest_host(torch.from_numpy(q).to(dev)) == ref.digest(q.tobytes())


@pytest.mark.parametrize('n', [4097, (64 << 10) + 3])
def test_a_flipped_bit_and_two_swapped_words_change_both_words(dev, n):
    buf = ref.random_bytes(n, seed=4)
    s0, x0 = ops.bytes_digest_host(torch.from_numpy(buf).to(dev))
    for at in (0, n // 2, n - 1):
        flipped = buf.copy()
        flipped[at] ^= 0x08
        s1, x1 = ops.bytes_digest_host(torch.from_numpy(flipped).to(dev))
        assert s1 != s0 and x1 != x0 and (s1, x1) == ref.digest(flipped)
    swapped = buf.copy()
    swapped[8:16], swapped[n // 2 // 8 * 8:n // 2 // 8 * 8 + 8] = buf[n // 2 // 8 * 8:n // 2 // 8 * 8 + 8], buf[8:16]
    s2, x2 = ops.bytes_digest_host(torch.from_numpy(swapped).to(dev))
    assert s2 != s0 and x2 != x0 and (s2, x2) == ref.digest(swapped)


def test_digest_replays_from_a_captured_graph(dev):
    first, second = ref.random_bytes((64 << 10) + 3, seed=7), ref.random_bytes((64 << 10) + 3, seed=8)
    t = torch.from_numpy(first).to(dev)
    side = _lib.private_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.bytes_digest(t)                                                     # allocator warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = ops.bytes_digest(t)                                           # no host read inside: the capture would fail
    torch.cuda.current_stream().wait_stream(side)
    for buf in (first, second, first):
        t.copy_(torch.from_numpy(buf))
        out.view(torch.int64).fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert tuple(int(v) for v in out.view(torch.int64).cpu().numpy().view(np.uint64)) == ref.digest(buf)


# ------------------------------------------------------------------------------------------------ round trips
def exp_for(Tl=1, **kw):
    return types.SimpleNamespace(Tm=TM, Tl=Tl, input_size=CANVAS, test_size=CANVAS, num_classes=3, window=-50, aggregation='micro_sum', **kw)


def gen1_recordings():
    return data.synth_gen1_recordings(3, 4, n_events=5000, sensor_hw=SENSOR)


BUILDERS = {
    'window': lambda dev, shard: data.Gen1WindowStore(gen1_recordings(), 1, (-50_000, 0), dev, sensor_hw=SENSOR, shard=shard),
    'packed_window': lambda dev, shard: data.Gen1PackedWindowStore(gen1_recordings(), 1, (-50_000, 0), dev, sensor_hw=SENSOR, shard=shard),
    'gen4': lambda dev, shard: data.Gen4Store(data.synth_gen4_recordings(3, 7, sensor_hw=(24, 32)), TM, dev, sensor_hw=(24, 32), shard=shard),
    'packed_gen4': lambda dev, shard: data.Gen4PackedStore(data.synth_gen4_recordings(3, 7, sensor_hw=(24, 32)), TM, dev, sensor_hw=(24, 32),
                                                           shard=shard),
    'atis': lambda dev, shard: data.NCaltechStore(data.synth_ncaltech_recordings(6, 3000, sensor_hw=SENSOR), 1, None, dev, sensor_hw=SENSOR,
                                                  shard=shard),
}
LOADERS = {'window': data.Gen1StoreLoader, 'packed_window': data.Gen1StoreLoader, 'gen4': data.Gen4StoreLoader, 'packed_gen4': data.Gen4StoreLoader,
           'atis': data.NCaltechStoreLoader}
_BUILT = {}


def built(dev, kind, shard=None, trimmed=True):
    """the store of a kind, built once for the module and left unchanged (an untrimmed store is a build of its own)"""
    key = (kind, shard, trimmed)
    if key not in _BUILT:
        store = BUILDERS[kind](dev, shard)
        _BUILT[key] = store.trim() if trimmed and hasattr(store, 'trim') else store
    return _BUILT[key]


def assert_same_device_store(got, want, dev):
    assert type(got) is type(want) and len(got) == len(want) and got.device == want.device == dev
    for k, v in want.host.items():
        assert np.array_equal(v, got.host[k]) and v.dtype == got.host[k].dtype and torch.equal(getattr(got, k), getattr(want, k))
    fields = type(want)._snapshot_fields
    assert fields['device']
    for k in fields['device']:
        a, b = getattr(want, k), getattr(got, k)
        assert (a is None and b is None) or (b.device == dev and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)), k
    for k in fields['scalars'] + fields['lists']:
        assert getattr(got, k) == getattr(want, k), k
    assert got.sample_names == want.sample_names and got.shard == want.shard and np.array_equal(got.owned_samples, want.owned_samples)
    assert (want.sample_rank is None and got.sample_rank is None) or np.array_equal(want.sample_rank, got.sample_rank)
    assert not hasattr(got, '_arena')
    if hasattr(got, 'trim'):
        assert got.trim() is got
    if hasattr(want, 'used_bytes'):
        assert got.capacity_bytes == got.used_bytes == want.used_bytes
    if hasattr(want, 'held_first'):
        assert torch.equal(got.held_first, want.held_first) and torch.equal(got.held_lo, want.held_lo)
    for i in range(len(want)):
        assert np.array_equal(got.raw_labels(i), want.raw_labels(i))


def assert_same_batch(kind, got, want, dev):
    """frames and targets of the loader's first batch, from both stores"""
    exp = exp_for()
    a, b = LOADERS[kind](exp, 2, store=want, seed=1), LOADERS[kind](exp, 2, store=got, seed=1)
    batch = a.batches(0)[0]
    assert all(np.array_equal(u, v) for u, v in zip(batch, b.batches(0)[0]))
    got.check_owned(batch[0])
    idx, par, *perm = (torch.from_numpy(v).to(dev) for v in batch)
    fw, fg = want.frames(idx, par, exp), got.frames(idx, par, exp)
    assert torch.equal(fw, fg) and fw.any() and fw.shape[0] == 2
    assert torch.equal(want.targets(idx, par, *perm, CANVAS), got.targets(idx, par, *perm, CANVAS))
    return batch[0]


@pytest.mark.parametrize('kind', list(BUILDERS))
def test_round_trip_on_the_device(dev, kind, tmp_path):
    want = built(dev, kind)
    path = want.save(str(tmp_path / 'store.eas'))
    got = data.load_store(path, dev, expect_shard=None)
    assert_same_device_store(got, want, dev)
    assert_same_batch(kind, got, want, dev)
    header, arrays = ref.read_snapshot(path)                                    # the layout and the digests, read independently
    for k in type(want)._snapshot_fields['device']:
        assert np.array_equal(arrays[k].view(np.uint8).reshape(-1), getattr(want, k).cpu().reshape(-1).view(torch.uint8).numpy())


@pytest.mark.parametrize('kind', ['window', 'packed_window', 'packed_gen4'])
def test_an_untrimmed_store_is_saved_at_its_used_size(dev, kind, tmp_path):
    loose, tight = built(dev, kind, trimmed=False), built(dev, kind)
    assert loose.capacity_bytes > loose.used_bytes == tight.used_bytes
    path = loose.save(str(tmp_path / 'loose.eas'))
    assert open(path, 'rb').read() == open(tight.save(str(tmp_path / 'tight.eas')), 'rb').read()
    assert loose.capacity_bytes > loose.used_bytes                               # saving changes nothing
    got = data.load_store(path, dev)
    assert_same_device_store(got, tight, dev)
    assert_same_batch(kind, got, loose, dev)


@pytest.mark.parametrize('kind', list(BUILDERS))
def test_round_trip_of_a_shard(dev, kind, tmp_path):
    want = built(dev, kind, shard=(0, 2))
    path = want.save(str(tmp_path / 'shard.eas'))
    got = data.load_store(path, dev, expect_shard=(0, 2))
    assert_same_device_store(got, want, dev)
    assert got.sharded and 0 < len(got.owned_samples) < len(got)
    drawn = assert_same_batch(kind, got, want, dev)
    assert got.owns(drawn).all()
    others = np.setdiff1d(np.arange(len(got)), got.owned_samples)
    with pytest.raises(IndexError):
        got.check_owned(others[:1])
    with pytest.raises(data.SnapshotError, match='shard'):
        data.load_store(path, dev, expect_shard=(1, 2))
    with pytest.raises(data.SnapshotError, match='shard'):
        data.load_store(path, dev, expect_shard=None)


@pytest.mark.parametrize('kind', ['packed_window', 'packed_gen4', 'atis'])
def test_chunks_of_4096_bytes_give_the_one_chunk_load(dev, kind, tmp_path):
    """more than three chunks and no multiple of the chunk: both staging buffers are used again, and the last chunk is short"""
    want = built(dev, kind)
    big = {'packed_window': 'payload', 'packed_gen4': 'payload', 'atis': 'records'}[kind]
    nbytes = getattr(want, big).numel()
    assert nbytes > 3 * 4096
    if nbytes % 4096 == 0:                                                      # (a payload is whole units: the second section then is no multiple)
        other = {'packed_window': 'sample_ranges', 'packed_gen4': 'rows'}[kind]
        assert (getattr(want, other).numel() * getattr(want, other).element_size()) % 4096 != 0
    one = want.save(str(tmp_path / 'one.eas'))
    small = want.save(str(tmp_path / 'small.eas'), chunk_bytes=4096)
    assert open(one, 'rb').read() == open(small, 'rb').read()
    a, b = data.load_store(one, dev), data.load_store(small, dev, chunk_bytes=4096)
    assert_same_device_store(b, a, dev)
    assert_same_device_store(b, want, dev)
    assert_same_batch(kind, b, want, dev)
    c = data.load_store(small, dev, chunk_bytes=4096 + 16)                      # a chunk that is no power of two
    assert_same_device_store(c, want, dev)


def test_a_flipped_byte_in_a_device_section_is_found_on_the_device(dev, tmp_path):
    want = built(dev, 'packed_window')
    path = want.save(str(tmp_path / 'store.eas'))
    e = next(e for e in ref.read_snapshot(path)[0]['sections'] if e['name'] == 'payload')
    assert e['where'] == 'device' and e['nbytes'] > 0
    raw = bytearray(open(path, 'rb').read())
    raw[e['offset'] + e['nbytes'] - 1] ^= 0x80
    with open(path, 'wb') as f:
        f.write(bytes(raw))
    with pytest.raises(data.SnapshotError, match="'payload'") as err:
        data.load_store(path, dev, chunk_bytes=4096)
    assert path in str(err.value) and isinstance(err.value, ValueError)


# ------------------------------------------------------------------------------------------------ exp.store_cache, end to end
def test_first_batch_from_a_cached_packed_window_store_equals_the_built_ones(dev, tmp_path, monkeypatch):
    root, cache = tmp_path / 'gen1', str(tmp_path / 'cache')
    recs = gen1_recordings()
    for d, part in (('train', recs[:2]), ('val', recs[2:])):
        os.makedirs(str(root / d))
        for name, dat, rows in part:
            dat.tofile(str(root / d / f'{name}_td.dat'))
            np.save(str(root / d / f'{name}_bbox.npy'), rows)

    def make_exp():
        return exp_for(data_dir=str(root), store_cache=cache, store_records='windows', store_events='packed')
    first = data.Gen1StoreLoader(make_exp(), 4, seed=2)
    assert type(first.store) is data.Gen1PackedWindowStore and hasattr(first.store, '_arena')
    (name,) = os.listdir(cache)
    assert name.startswith('dat_store_train_') and name.endswith('.eas') and ref.read_snapshot(os.path.join(cache, name))[0]['key']['cls'] == \
        'Gen1PackedWindowStore'
    monkeypatch.setattr(data.Gen1PackedWindowStore, 'from_directories', classmethod(lambda *a, **k: 1 / 0))
    second = data.Gen1StoreLoader(make_exp(), 4, seed=2)
    assert second.store is not first.store and not hasattr(second.store, '_arena')
    assert_same_device_store(second.store, first.store, dev)
    (fa, ta), (fb, tb) = next(iter(first)), next(iter(second))
    assert torch.equal(fa, fb) and torch.equal(ta, tb) and fa.any() and fa.shape == (4, 1, TM, 2, *CANVAS)
