"""CPU-only tests of the 1 Mpx store in packed rows: the numpy statement of the format (tests/packed_store_ref.py) round-trips and its byte
count obeys the bounds the format's arithmetic gives; the four entries are declared, exported, bound and refuse bad arguments before any
launch; ``exp.store_sums`` selects the class; ``data.Gen4PackedStore`` on host tensors has the parent's tables and no payload; a sensor
wider than 1024 pixels is refused."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import gen4_store_ref
import packed_store_ref as ref
import eas_snn_amd
from eas_snn_amd import data, ops

INVALID, UNSUPPORTED = -1, -2
SHAPES = [(6, 16), (5, 40), (4, 37), (2, 1024)]


@pytest.mark.parametrize('H,W', SHAPES)
def test_checker_round_trips(H, W):
    f = ref.fields(H, W)
    assert not f[0].any() and (f[1] == 255).all() and f[2].max() == 256 and f[3].max() == 65025 and f[3, 0, H - 1, W - 1] == 65025
    table, payload = ref.encode(f)
    assert table.dtype == np.int64 and table.shape == (7, 2, H, 3) and payload.dtype == np.uint8
    assert np.array_equal(ref.decode(table, payload, W), f)
    need, tab = ref.packed_bytes(f)
    assert len(payload) == need and tab == table.nbytes
    words = table.view(np.uint64)
    G = (W + 15) // 16
    assert not words[0, ..., :2].any() and (words[0, ..., 2] == 0).all()                    # zeros: no bit, no unit
    assert (words[1, ..., 0] == (1 << G) - 1).all() and not words[1, ..., 1].any()          # 255 everywhere: every group narrow
    assert np.count_nonzero(words[2, ..., 0]) == 1 and np.count_nonzero(words[2, ..., 1]) == 1
    assert int(words[3, 0, H - 1, 1]) == 1 << (G - 1)                                       # the last group of the last row is wide
    # rows follow each other without gaps, in row order
    flat = words.reshape(-1, 3)
    units = np.array([ref.popcount(a) + ref.popcount(b) for a, b, _ in flat])
    assert np.array_equal(flat[:, 2].astype(np.int64), np.cumsum(units) - units)
    # a chunk packed behind unit 5 differs in its offsets only
    moved, same = ref.encode(f[3:], unit_offset=5)
    assert np.array_equal(same, payload[16 * int(flat[3 * 2 * H, 2]):]) and np.array_equal(ref.decode(moved, same, W, unit_offset=5), f[3:])


def test_byte_count_obeys_the_bounds():
    """(1) never larger than the u16 store (rows counted in whole groups: the u16 store itself where W % 16 == 0) plus 24 bytes per row;
    (2) no sum above 255: table + payload at least 1.92 times smaller than the u16 store at W = 640; (3) an all-zero group costs nothing"""
    rng = np.random.default_rng(7)
    H, W = 360, 640
    for lam, active in ((0.3, 1.0), (0.3, 0.4), (0.3, 0.15), (40.0, 1.0)):
        f = rng.poisson(lam, (1, 2, H, W)).astype(np.uint16)
        keep = rng.random((1, 2, H, W // 16)) < active
        f *= np.repeat(keep, 16, axis=3)
        if lam > 1:
            f[0, :, ::7, ::5] = 300                                                           # wide groups among narrow ones
        payload, table = ref.packed_bytes(f)
        top = ref.groups_of(f).max(axis=2)
        assert payload == 16 * (int((top > 0).sum()) + int((top > 255).sum()))                # (3)
        assert payload <= f.nbytes and table == 24 * 2 * H                                    # (1)
        if f.max() <= 255:
            assert (payload + table) * 1.92 <= f.nbytes, (lam, active)                        # (2)
    worst = np.full((1, 2, 4, 640), 65025, dtype=np.uint16)
    assert ref.packed_bytes(worst)[0] == worst.nbytes
    for H, W in SHAPES:                                                                       # widths that are no multiple of 16
        f = ref.fields(H, W)
        payload, table = ref.packed_bytes(f)
        assert payload <= 7 * 2 * H * ((W + 15) // 16) * 32 and table == 24 * 7 * 2 * H


def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    eas_snn_amd._lib._bind_host_hip_runtime()
    handle = ctypes.CDLL(eas_snn_amd._lib.LIB_PATH)
    C = ctypes
    P = C.c_void_p
    want = {'eas_count_rows_measure': (C.c_int, [P, C.c_int64, C.c_int, C.c_int, P, P]),
            'eas_count_rows_pack': (C.c_int, [P, C.c_int64, C.c_int, C.c_int, P, P, C.c_int64, C.c_int64, P]),
            'eas_count_rows_unpack': (C.c_int, [P, P, C.c_int64, C.c_int64, C.c_int, C.c_int, P, P]),
            'eas_packed_store_frames': (C.c_int, [P, P, C.c_int64, C.c_int64, P, P, P] + [C.c_int] * 6 + [P] * 3)}
    for n, proto in want.items():
        assert n in declared and hasattr(handle, n) and eas_snn_amd._lib.PROTOTYPES[n] == proto
    assert sorted(eas_snn_amd._lib.PROTOTYPES) == sorted(declared)
    assert eas_snn_amd._lib.ABI_VERSION == 9 and eas_snn_amd.hip_library().eas_abi_version() == 9          # purely additive
    for name in ('count_rows_pack', 'count_rows_unpack', 'packed_store_frames'):
        assert hasattr(ops, name)
    assert hasattr(data, 'Gen4PackedStore') and issubclass(data.Gen4PackedStore, data.Gen4Store) and data.STORE_SUMS == ('u16', 'packed')


def test_bad_arguments_are_refused_before_any_launch():
    """every call below returns from the argument checks: no device is touched (the pointers are made-up addresses)"""
    lib = eas_snn_amd.hip_library()
    good = dict(sums=0x10000, n=3, H=18, W=32, table=0x20000, payload=0x30000, lo=4, hi=9, units=9)

    def measure(**kw):
        a = dict(good, **kw)
        return lib.eas_count_rows_measure(a['sums'], a['n'], a['H'], a['W'], a['table'], None)

    def pack(**kw):
        a = dict(good, **kw)
        return lib.eas_count_rows_pack(a['sums'], a['n'], a['H'], a['W'], a['table'], a['payload'], a['lo'], a['hi'], None)

    def unpack(**kw):
        a = dict(good, **kw)
        return lib.eas_count_rows_unpack(a['table'], a['payload'], a['units'], a['n'], a['H'], a['W'], a['sums'], None)
    for fn in (measure, pack, unpack):
        for kw in (dict(sums=None), dict(table=None), dict(n=-1), dict(H=0), dict(W=0), dict(sums=0x10008), dict(table=0x20004),
                   dict(sums=0x10001, W=30)):
            assert fn(**kw) == INVALID, (fn.__name__, kw)
        assert fn(W=1040) == UNSUPPORTED and fn(W=1025, n=0) == UNSUPPORTED and fn(n=0) == 0 and fn(n=0, W=1024) == 0
        assert fn(n=0, W=30, sums=0x10002) == 0                              # rows that are not 16-byte aligned: the element path asks for less
    for kw in (dict(payload=None), dict(payload=0x30008), dict(lo=-1), dict(lo=9, hi=4)):
        assert pack(**kw) == INVALID, kw
    assert pack(payload=None, lo=4, hi=4) == 0                               # nothing to write: no arena needed, no launch
    for kw in (dict(payload=None), dict(payload=0x30008), dict(units=-1)):
        assert unpack(**kw) == INVALID, kw
    good = dict(table=0x10000, payload=0x70000, units=12, R=8, first=0x20000, lo=0x30000, params=0x40000, B=2, Tm=3, H=18, W=32, Hc=32, Wc=48,
                out=0x50000, flags=0x60000)

    def frames(**kw):
        a = dict(good, **kw)
        return lib.eas_packed_store_frames(a['table'], a['payload'], a['units'], a['R'], a['first'], a['lo'], a['params'], a['B'], a['Tm'], a['H'],
                                           a['W'], a['Hc'], a['Wc'], a['out'], a['flags'], None)
    for kw in (dict(table=None), dict(first=None), dict(out=None), dict(R=0), dict(B=0), dict(Tm=0), dict(H=0), dict(W=0), dict(Hc=0), dict(Wc=0),
               dict(table=0x10004), dict(payload=0x70008), dict(payload=None), dict(units=-1), dict(out=0x50004), dict(first=0x20004),
               dict(lo=0x30004), dict(params=0x40002), dict(flags=0x60001)):
        assert frames(**kw) == INVALID, kw
    for kw in (dict(Wc=40), dict(W=1040), dict(W=1025, Wc=2048), dict(W=1024, Wc=8192)):          # the last: no band fits the LDS
        assert frames(**kw) == UNSUPPORTED, kw


def test_cpu_tensors_raise():
    sums, table, payload = torch.zeros(3, 2, 4, 16, dtype=torch.uint16), torch.zeros(3, 2, 4, 3, dtype=torch.int64), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.count_rows_pack(sums, table, payload, 0)
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.count_rows_unpack(table, payload, 16)
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.packed_store_frames(table, payload, torch.zeros(2, dtype=torch.int64), 2, 32, 32, W=16)


@pytest.fixture(scope='module')
def recordings():
    return gen4_store_ref.fixture_recordings(load_golden('gen4_store'))


def test_packed_store_on_the_host_has_the_parents_tables(recordings):
    tab = gen4_store_ref.tables(recordings, 3, 2, (12, 16))
    store = data.Gen4PackedStore(recordings, 3, 'cpu', sensor_hw=(12, 16), chunk=2)
    parent = data.Gen4Store(recordings, 3, 'cpu', sensor_hw=(12, 16), chunk=2)
    for k in ('rep_offsets', 'group_first', 'group_lo', 'boxes', 'group_start'):
        assert torch.equal(getattr(store, k), getattr(parent, k)) and np.array_equal(store.host[k], tab[k]), k
    assert store.sample_names == parent.sample_names == tab['sample_names'] and store.names == parent.names and len(store) == 7
    assert store.sums is None and store.rows is None and store.payload is None and store.used_bytes == 0
    assert all(np.array_equal(store.raw_labels(i), parent.raw_labels(i)) for i in range(7))
    half = data.Gen4PackedStore(recordings, 3, 'cpu', sensor_hw=(12, 16), shard=(1, 2))
    want = data.Gen4Store(recordings, 3, 'cpu', sensor_hw=(12, 16), shard=(1, 2))
    assert half.shard == (1, 2) and np.array_equal(half.owned_samples, want.owned_samples) and torch.equal(half.held_first, want.held_first)


def test_a_sensor_wider_than_64_groups_is_refused():
    recs = data.synth_gen4_recordings(1, 2, (2, 1040), 2, 3)
    with pytest.raises(ValueError, match='1040'):
        data.Gen4PackedStore(recs, 3, 'cpu', sensor_hw=(2, 1040), nbins=2)
    assert len(data.Gen4Store(recs, 3, 'cpu', sensor_hw=(2, 1040), nbins=2)) == 1             # the u16 store takes it
    with pytest.raises(ValueError, match='64 groups'):
        ref.encode(np.zeros((1, 2, 2, 1040), dtype=np.uint16))
    data.Gen4PackedStore(data.synth_gen4_recordings(1, 2, (2, 1024), 2, 3), 3, 'cpu', sensor_hw=(2, 1024), nbins=2)


def test_store_sums_selects_the_class():
    def exp(**kw):
        return types.SimpleNamespace(Tm=3, Tl=1, input_size=(32, 48), test_size=(32, 48), num_classes=3, store_recordings=(2, 6), **kw)
    e = exp()
    plain = data.hist_store_for(e, device='cpu')
    assert type(plain) is data.Gen4Store
    e.store_sums = 'packed'
    packed = data.hist_store_for(e, device='cpu')
    assert type(packed) is data.Gen4PackedStore and data.hist_store_for(e, device='cpu') is packed         # part of the cache key
    assert packed.sample_names == plain.sample_names
    e.store_sums = 'u16'
    assert data.hist_store_for(e, device='cpu') is plain
    for bad in ('u8', 'Packed', None):
        with pytest.raises(ValueError, match='store_sums'):
            data.hist_store_for(exp(store_sums=bad), device='cpu')
    from yolox.exp import get_exp
    g = get_exp(None, 'e-yolox-s')
    g.merge(['input_size', '(32, 48)', 'test_size', '(32, 48)', 'num_classes', '3'])
    g.train_input, g.store_recordings, g.store_sums = 'hist_store', (2, 12), 'bogus'
    with pytest.raises(ValueError, match='store_sums'):
        g.get_data_loader(4, False)
