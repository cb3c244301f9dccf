"""CPU-only tests of the Gen1 window store in packed records: the numpy statement of the format (tests/packed_records_ref.py) gives the
records back byte for byte and its byte count obeys the bounds the format states; the kinds of block it tells apart; what the recordings
of the store tests keep; the five entries are declared, exported, bound and refuse bad arguments before any launch; ``exp.store_events``
selects the class and refuses what it cannot do before any device work."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

import packed_records_ref as ref
import window_store_ref
import eas_snn_amd
from eas_snn_amd import data, ops

INVALID, UNSUPPORTED = -1, -2
SENSORS = [(240, 304), (12, 20), (12, 16), (12, 17)]
COUNTS = [1, 63, 64, 65, 64 * 1024 + 1]


def test_field_widths():
    assert ref.widths(240, 304) == (9, 8, 14) == ops.records_widths(240, 304)
    assert ref.widths(12, 16) == (4, 4, 23) and ref.widths(12, 17) == (5, 4, 22) and ref.widths(1, 1) == (1, 1, 29) == ops.records_widths(1, 1)
    assert ref.widths(2048, 4096) == (12, 11, 8) == ops.records_widths(2048, 4096)
    for H, W in ((2049, 4096), (4096, 4096), (16384, 16384), (240, 16385)):
        with pytest.raises(ValueError):
            ref.widths(H, W)
        with pytest.raises(ValueError):
            ops.records_widths(H, W)


@pytest.mark.parametrize('H,W', SENSORS)
def test_checker_round_trips_and_obeys_the_bounds(H, W):
    for n in COUNTS:
        rec, kinds = ref.records_of_every_kind(H, W, n, seed=n)
        nb = (n + 63) // 64
        base, wide = ref.block_kinds(rec, H, W)
        whole = n // 64                                                    # the kinds are stated for whole blocks
        assert np.array_equal(wide[:whole], ref.expected_wide(kinds, H, W)[:whole]) and len(wide) == nb == len(kinds)
        table, payload = ref.pack(rec, H, W)
        assert table.dtype == np.uint32 and table.shape == (nb, 2) and payload.dtype == np.uint8
        assert np.array_equal(ref.unpack(table, payload, 0, n, H, W), rec)                                  # byte for byte
        assert np.array_equal(ref.unpack(table, payload, n - 1, nb * 64, H, W), np.repeat(rec[-1:], nb * 64 - n + 1, 0))    # the padding
        need, tab = ref.packed_bytes(rec, H, W)
        assert len(payload) == need and tab == table.nbytes == 8 * nb
        assert need + tab <= 8 * 64 * nb + 8 * nb                                                         # raw (in whole blocks) + 8 bytes per block
        assert need + tab == 264 * nb + 256 * int(wide.sum())
        # places: an exclusive scan of the units; a call behind unit 5 differs in its places only
        units = 1 + wide.astype(np.int64)
        assert np.array_equal(table[:, 1] & 0x7fffffff, np.cumsum(units) - units) and np.array_equal(table[:, 1] >> 31, wide)
        assert np.array_equal(table[:, 0], base)
        moved, same = ref.pack(rec, H, W, unit_offset=5)
        assert np.array_equal(same, payload) and np.array_equal((moved[:, 1] & 0x7fffffff) - 5, table[:, 1] & 0x7fffffff)
        if n > 64:
            a, e = 37, min(n, 64 * 9 + 11)
            assert np.array_equal(ref.unpack(moved, same, a, e, H, W, unit_offset=5), rec[a:e])


def test_no_wide_block_is_264_bytes_per_block():
    rng = np.random.default_rng(3)
    n = 64 * 50
    t = 1_000_000 + np.cumsum(rng.integers(0, 200, n))                      # 64 records within 12.8 ms at most
    rec = np.stack([t.astype(np.uint32), ref.word(rng.integers(0, 304, n), rng.integers(0, 240, n), rng.integers(0, 2, n))], 1)
    payload, table = ref.packed_bytes(rec, 240, 304)
    assert payload + table == 264 * 50 and (payload + table) / rec.nbytes == 0.515625
    worst = rec.copy()
    worst[::64, 1] |= 1 << 29                                               # every block wide: raw + 8 bytes per block, 1.6 %
    payload, table = ref.packed_bytes(worst, 240, 304)
    assert payload == worst.nbytes and table == 8 * 50 and (payload + table) / worst.nbytes == 1.015625


def test_padding_never_turns_a_narrow_block_wide():
    """a last block of one record up to 63 is as wide as those records alone make it"""
    for kind in ('random', 'span_max', 'backwards', 'equal', 'x_top'):
        blk = ref.kind_block(kind, 240, 304, 5_000_000, np.random.default_rng(1))
        for n in (1, 2, 33, 63):
            assert not ref.block_kinds(blk[:n], 240, 304)[1][0], (kind, n)


@pytest.mark.parametrize('Tl,narrow,wide', [(1, 1509, 22), (2, 3041, 4)])
def test_the_store_tests_recordings_keep_blocks_of_both_kinds(Tl, narrow, wide):
    """a condition on the inputs of the GPU store tests: with every recording on a fresh block, the records the window store keeps of
    ``window_store_ref.recordings()`` make narrow and wide blocks"""
    recs = window_store_ref.recordings()
    lay = window_store_ref.layout(recs, Tl)
    rows = np.concatenate([np.ascontiguousarray(dat[data.parse_dat_header(dat)[0]:]).view('<u4').reshape(-1, 2) for _, dat, _ in recs])
    kept = rows[lay['keep']]
    got = [0, 0]
    for a, e in zip(lay['file_offsets'][:-1], lay['file_offsets'][1:]):
        w = ref.block_kinds(kept[a:e], *window_store_ref.SENSOR)[1]
        got[0] += int((~w).sum())
        got[1] += int(w.sum())
    assert got == [narrow, wide]


def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    eas_snn_amd._lib._bind_host_hip_runtime()
    handle = ctypes.CDLL(eas_snn_amd._lib.LIB_PATH)
    C = ctypes
    P, L, I = C.c_void_p, C.c_int64, C.c_int
    want = {'eas_records_pack_measure': (I, [P, L, I, I, P, P]),
            'eas_records_pack': (I, [P, L, I, I, P, P, L, L, P]),
            'eas_records_unpack': (I, [P, L, P, L, L, L, I, I, P, P, P]),
            'eas_event_histogram_packed_ranges': (I, [P, L, P, L, P, I, I, I, I, P, P, P, P]),
            'eas_event_latest_surface_packed_ranges': (I, [P, L, P, L, P, I, I, I, I, C.c_double, P, P, P, P])}
    for n, proto in want.items():
        assert n in declared and hasattr(handle, n) and eas_snn_amd._lib.PROTOTYPES[n] == proto, n
    assert sorted(eas_snn_amd._lib.PROTOTYPES) == sorted(declared)
    assert eas_snn_amd._lib.ABI_VERSION == 9 and eas_snn_amd.hip_library().eas_abi_version() == 9          # purely additive
    for name in ('records_pack', 'records_unpack', 'event_histogram_packed_ranges', 'event_latest_surface_packed_ranges', 'PackedArenaFull'):
        assert hasattr(ops, name)
    assert hasattr(data, 'packed_ranges_to_frames') and issubclass(data.Gen1PackedWindowStore, data.Gen1WindowStore)
    assert data.STORE_RECORDS == ('all', 'windows') and data.STORE_EVENTS == ('dat', 'packed')


def test_bad_arguments_are_refused_before_any_launch():
    """every call below returns from the argument checks: no device is touched (the pointers are made-up addresses)"""
    lib = eas_snn_amd.hip_library()
    good = dict(rec=0x10000, n=130, H=240, W=304, table=0x20000, payload=0x30000, lo=4, hi=9, nb=3, units=9, a=5, e=150, out=0x40000, flags=0x50000)

    def measure(**kw):
        a = dict(good, **kw)
        return lib.eas_records_pack_measure(a['rec'], a['n'], a['H'], a['W'], a['table'], None)

    def pack(**kw):
        a = dict(good, **kw)
        return lib.eas_records_pack(a['rec'], a['n'], a['H'], a['W'], a['table'], a['payload'], a['lo'], a['hi'], None)

    def unpack(**kw):
        a = dict(good, **kw)
        return lib.eas_records_unpack(a['table'], a['nb'], a['payload'], a['units'], a['a'], a['e'], a['H'], a['W'], a['out'], a['flags'], None)
    for fn in (measure, pack):
        for kw in (dict(rec=None), dict(table=None), dict(n=-1), dict(H=0), dict(W=0), dict(rec=0x10004), dict(table=0x20004)):
            assert fn(**kw) == INVALID, (fn.__name__, kw)
        for kw in (dict(H=4096, W=4096), dict(H=2049, W=4096), dict(W=16385), dict(H=16385, W=2, n=0)):                   # DB < 8, a 15-bit side
            assert fn(**kw) == UNSUPPORTED, (fn.__name__, kw)
        assert fn(n=0) == 0 and fn(n=0, rec=None) == 0 and fn(H=2048, W=4096, n=0) == 0
    for kw in (dict(payload=None), dict(payload=0x30008), dict(lo=-1), dict(lo=9, hi=4), dict(hi=(1 << 31) + 1)):
        assert pack(**kw) == INVALID, kw
    assert pack(payload=None, lo=4, hi=4) == 0                               # nothing to write: no arena needed, no launch
    for kw in (dict(table=None), dict(table=0x20004), dict(payload=None), dict(payload=0x30008), dict(units=-1), dict(nb=-1), dict(a=-1),
               dict(a=151), dict(e=193), dict(out=None), dict(out=0x40004), dict(flags=0x50002), dict(H=0), dict(W=0), dict(units=(1 << 31) + 1)):
        assert unpack(**kw) == INVALID, kw
    assert unpack(H=4096, W=4096) == UNSUPPORTED
    good = dict(table=0x10000, nb=8, payload=0x70000, units=12, ranges=0x20000, B=2, ns=3, H=18, W=32, out=0x50000, oob=0x60000, flags=0x60040, tau=5e4)

    def counts(**kw):
        a = dict(good, **kw)
        return lib.eas_event_histogram_packed_ranges(a['table'], a['nb'], a['payload'], a['units'], a['ranges'], a['B'], a['ns'], a['H'], a['W'],
                                                     a['out'], a['oob'], a['flags'], None)

    def surfaces(**kw):
        a = dict(good, **kw)
        return lib.eas_event_latest_surface_packed_ranges(a['table'], a['nb'], a['payload'], a['units'], a['ranges'], a['B'], a['ns'], a['H'],
                                                          a['W'], a['tau'], a['out'], a['oob'], a['flags'], None)
    for fn in (counts, surfaces):
        for kw in (dict(table=None), dict(payload=None), dict(ranges=None), dict(out=None), dict(nb=-1), dict(units=-1), dict(B=0), dict(ns=0),
                   dict(H=0), dict(W=0), dict(table=0x10004), dict(payload=0x70008), dict(flags=0x60042), dict(units=(1 << 31) + 1)):
            assert fn(**kw) == INVALID, (fn.__name__, kw)
        for kw in (dict(B=65536), dict(H=4096, W=4096)):
            assert fn(**kw) == UNSUPPORTED, (fn.__name__, kw)
    for tau in (0.0, -1.0, float('nan')):
        assert surfaces(tau=tau) == INVALID


def test_cpu_tensors_raise():
    rec, table, payload = torch.zeros(8 * 70, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(1024, dtype=torch.uint8)
    ranges = torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.records_pack(rec, table, payload, 0, 240, 304)
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.records_unpack(table, payload, 0, 70, 240, 304)
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.event_histogram_packed_ranges(table, payload, ranges, 2, 240, 304)
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.event_latest_surface_packed_ranges(table, payload, ranges, 2, 240, 304)
    for fn in (lambda: ops.records_pack(rec, table, payload, 0, 4096, 4096), lambda: ops.records_unpack(table, payload, 0, 70, 4096, 4096),
               lambda: ops.event_histogram_packed_ranges(table, payload, ranges, 2, 4096, 4096)):
        with pytest.raises(ValueError, match='bits'):                        # the geometry is refused first, on the host
            fn()


def test_store_events_selects_the_class_and_refuses_before_any_device_work():
    def exp(**kw):
        return types.SimpleNamespace(Tm=3, Tl=1, window=-20, input_size=(32, 48), test_size=(32, 48), num_classes=2,
                                     store_recordings=(2, 4, 0), **kw)       # recordings without events: nothing for a device to do
    plain = data.gen1_store_for(exp(), device='cpu')
    assert type(plain) is data.Gen1Store
    for kw in (dict(store_events='packed'), dict(store_events='packed', store_records='all'), dict(store_events='Packed', store_records='windows'),
               dict(store_events=None), dict(store_events='dat', store_records='most')):
        with pytest.raises(ValueError, match='store_events' if kw.get('store_records') != 'most' else 'store_records'):
            data.gen1_store_for(exp(**kw), device='meta')                    # (a device nothing can run on: the refusal comes first)
    from yolox.exp import get_exp
    g = get_exp(None, 'e-yolox-s')
    assert g.store_events == 'dat'
    g.merge(['input_size', '(32, 48)', 'test_size', '(32, 48)', 'num_classes', '2'])
    g.train_input, g.store_recordings, g.store_events = 'dat_store', (2, 4, 0), 'packed'
    with pytest.raises(ValueError, match='store_events'):
        g.get_data_loader(4, False)                                          # store_records is 'all' by default


def test_a_sensor_that_leaves_no_room_for_the_time_is_refused():
    recs = data.synth_gen1_recordings(1, 2, 100, (4096, 4096))
    with pytest.raises(ValueError, match='bits'):
        data.Gen1PackedWindowStore(recs, 1, (-20_000, 0), 'cpu', sensor_hw=(4096, 4096), capacity_bytes=4096)
