"""CPU-only tests of the Gen1 store that keeps only the records its samples read: the numpy checker's union and mapping
(tests/window_store_ref.py) against a per-record mask on seeded ranges of every kind; what the checker says the store tests' recordings
keep; ``eas_records_gather`` is declared, exported, bound and refuses bad arguments before any launch; ``data.Gen1WindowStore`` takes its
recordings one at a time and shares the parent's tables; ``exp.store_records`` selects the class."""
import ctypes
import gc
import os
import re
import types
import weakref

import numpy as np
import pytest
import torch

from conftest import ROOT

import window_store_ref as ref
import eas_snn_amd
from eas_snn_amd import data, ops

INVALID = -1


@pytest.mark.parametrize('seed,n_records,m,max_len', [(0, 40, 1, None), (1, 40, 12, None), (2, 300, 60, None), (3, 1000, 200, None), (4, 7, 30, None),
                                                      (5, 2, 9, None), (6, 20_000, 400, 30)])
def test_checker_union_and_mapping_equal_a_per_record_mask(seed, n_records, m, max_len):
    rng = np.random.default_rng(seed)
    ranges = ref.random_ranges(rng, n_records, m, max_len)
    segments, seg_dst, mapped = ref.union(ranges)
    mask = np.zeros(n_records + 1, dtype=bool)
    for a, e in ranges:
        mask[a:e] = True
    # the segments are the maximal runs of the mask: sorted, disjoint, non-empty, not touching
    edges = np.flatnonzero(np.diff(np.r_[False, mask, False].astype(np.int8)))
    assert np.array_equal(segments.reshape(-1), edges) and segments.dtype == np.int64
    assert seg_dst[0] == 0 and np.array_equal(np.diff(seg_dst), segments[:, 1] - segments[:, 0]) and seg_dst[-1] == mask.sum()
    # compact[mapped] == full[ranges]: the k-th kept record is the k-th record of the mask
    kept = np.flatnonzero(mask)
    for (a, e), (ma, me) in zip(ranges, mapped):
        assert me - ma == e - a and 0 <= ma <= me <= len(kept)
        assert np.array_equal(kept[ma:me], np.arange(a, e))
    full = np.arange(n_records * 2).reshape(n_records, 2)
    assert np.array_equal(ref.gather(full, segments, seg_dst, np.full((len(kept) + 3, 2), -1), 2)[2:-1], full[kept])


def test_checker_on_the_kinds_by_hand():
    segments, seg_dst, mapped = ref.union([(5, 9), (1, 3), (3, 4), (6, 7), (5, 9), (20, 20), (8, 12), (0, 0), (30, 31)])
    assert segments.tolist() == [[1, 4], [5, 12], [30, 31]] and seg_dst.tolist() == [0, 3, 10, 11]
    assert mapped.tolist() == [[3, 7], [0, 2], [2, 3], [4, 5], [3, 7], [0, 0], [6, 10], [0, 0], [10, 11]]
    segments, seg_dst, mapped = ref.union(np.zeros((0, 2)))
    assert segments.shape == (0, 2) and seg_dst.tolist() == [0] and mapped.shape == (0, 2)
    assert ref.union([(4, 4)])[1].tolist() == [0]


@pytest.mark.parametrize('Tl', [1, 2])
def test_checker_layout_of_the_store_recordings(Tl):
    """the recordings of the GPU store tests: every window covers 20 ms of a 50 ms label period, so the store keeps less than it is given;
    the special recordings do what they are there for"""
    recs = ref.recordings()
    lay = ref.layout(recs, Tl)
    assert [r[0] for r in recs][1:3] == ['big', 'gap'] and lay['total'] == 3 * 20_000 + 250_000 + 8000 + 5000
    assert 0 < lay['kept'] < lay['total'] and lay['kept'] == len(lay['keep']) and lay['full_ranges'].shape == (6 * 3 + 6 + 4 + 2, Tl, 2)
    assert lay['kept'] < (0.45 if Tl == 1 else 0.85) * lay['total']
    offs = lay['file_offsets']
    assert offs[5] == offs[4] and offs[6] == offs[5] and (np.diff(offs)[[0, 1, 2, 3, 6]] > 0).all()      # no labels / no events: nothing kept
    full, comp = lay['full_ranges'], lay['sample_ranges']
    assert np.array_equal(full[..., 1] - full[..., 0], comp[..., 1] - comp[..., 0])
    for (a, e), (ma, me) in zip(full.reshape(-1, 2), comp.reshape(-1, 2)):
        assert np.array_equal(lay['keep'][ma:me], np.arange(a, e))
    # 'big': the label whose window starts at the first probe's time begins one record after the probe
    t_big = ref.record_times(recs[1][1])
    times = np.unique(recs[1][2]['t']).astype(np.int64)
    g = 6 + int(np.flatnonzero(times + ref.WINDOW[0] == t_big[125_000])[0])
    assert full[g, -1, 0] - 20_000 == 125_001 and t_big[125_000] >= times[g - 6] + ref.WINDOW[0]
    # 'gap' (samples 12 .. 15): the second label's window is empty and steps back onto events, the third one stays empty
    length = (full[..., 1] - full[..., 0])[12:16, -1]
    t_gap = ref.record_times(recs[2][1])
    assert length[1] > 0 and t_gap[full[13, -1, 1] - 270_000 - 1] < 1_105_000 and length[2] == 0 and length[0] > 0 and length[3] > 0
    assert (full[22:24, :, 1] == full[22:24, :, 0]).all()                                              # 'noevents' (samples 22, 23)


def test_entry_point_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    eas_snn_amd._lib._bind_host_hip_runtime()
    handle = ctypes.CDLL(eas_snn_amd._lib.LIB_PATH)
    n = 'eas_records_gather'
    assert n in declared and hasattr(handle, n) and n in eas_snn_amd._lib.PROTOTYPES
    assert sorted(eas_snn_amd._lib.PROTOTYPES) == sorted(declared)
    assert eas_snn_amd.hip_library().eas_abi_version() == eas_snn_amd._lib.ABI_VERSION                 # additive: the version stays
    for name in ('record_ranges_union', 'records_gather'):
        assert hasattr(ops, name)
    assert issubclass(data.Gen1WindowStore, data.Gen1Store) and data.STORE_RECORDS == ('all', 'windows')
    assert 'records.hip' in open(os.path.join(ROOT, 'eas_snn_amd', 'csrc', 'Makefile')).read()


def test_bad_arguments_are_refused_before_any_launch():
    """every call below returns from the argument checks: no device is touched (the pointers are made-up addresses)"""
    fn = eas_snn_amd.hip_library().eas_records_gather
    good = dict(src=0x10000, seg_src=0x20000, seg_dst=0x30000, S=3, total=10, dst=0x40000)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a['src'], a['seg_src'], a['seg_dst'], a['S'], a['total'], a['dst'], None)
    for kw in (dict(src=None), dict(seg_src=None), dict(seg_dst=None), dict(dst=None), dict(S=0), dict(S=-1), dict(total=-1),
               dict(src=0x10004), dict(seg_src=0x20004), dict(seg_dst=0x30001), dict(dst=0x40002)):
        assert call(**kw) == INVALID, kw
    assert call(total=0) == 0                                                                          # nothing to copy: no launch
    assert call(total=0, S=0) == INVALID and call(total=0, dst=None) == INVALID                        # bad arguments first


def test_cpu_tensors_raise():
    z = torch.zeros
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.record_ranges_union(z(3, 2, dtype=torch.int64))
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.records_gather(z(64, dtype=torch.uint8), z(1, 2, dtype=torch.int64), z(2, dtype=torch.int64), z(64, dtype=torch.uint8))


class HostWindowStore(data.Gen1WindowStore):
    """the store with the device steps of a recording replaced by the checker: the arena stays empty, everything else is the class's own"""

    def _window_ranges(self, area, times):
        t = np.ascontiguousarray(area).view('<u4').reshape(-1, 2)[:, 0].astype(np.int64)
        step = self.window[1] - self.window[0]
        local = [ref.events_ref.search_events(t, int(lt) + k * step, self.window, self.Tl) for lt in times for k in range(-self.Tl + 1, 1)]
        _, seg_dst, mapped = ref.union(local)
        return torch.from_numpy(mapped), int(seg_dst[-1])


def small_recordings():
    return data.synth_gen1_recordings(3, 6, n_events=500, sensor_hw=(24, 32), seed=4)


def test_recordings_are_taken_one_at_a_time():
    """a generator that counts the recordings handed out and not yet released never sees more than one"""
    live, peak, handed = [0], [0], [0]

    def release():
        live[0] -= 1

    def make(i):
        name, dat, rows = small_recordings()[i]
        dat = dat.copy()
        weakref.finalize(dat, release)
        live[0] += 1
        handed[0] += 1
        peak[0] = max(peak[0], live[0])
        return name, dat, rows

    def lazily():
        for i in range(3):
            gc.collect()
            yield make(i)
    store = HostWindowStore(lazily(), 2, (-20_000, 0), 'cpu', sensor_hw=(24, 32), capacity_bytes=3 * 500 * 8)
    gc.collect()
    assert handed[0] == 3 and peak[0] == 1 and live[0] == 0
    parent = data.Gen1Store(small_recordings(), 2, (-20_000, 0), 'cpu', sensor_hw=(24, 32))
    assert store.sample_names == parent.sample_names and store.names == parent.names and len(store) == len(parent) == 18
    for k in ('boxes', 'group_start', 'group_t', 'group_file'):
        assert torch.equal(getattr(store, k), getattr(parent, k)) and np.array_equal(store.host[k], parent.host[k])
    assert np.array_equal(store.raw_labels(7), parent.raw_labels(7)) and store.max_group_rows == parent.max_group_rows
    lay = ref.layout(small_recordings(), 2)
    assert store.total_records == lay['total'] == 1500 and store.kept_records == lay['kept'] and store.used_bytes == 8 * lay['kept']
    assert store.file_offsets.tolist() == lay['file_offsets'].tolist() and np.array_equal(store.sample_ranges.numpy(), lay['sample_ranges'])
    assert store.capacity_bytes == 12_000 and store.records.numel() == store.used_bytes
    assert store.trim() is store and store.capacity_bytes == store.used_bytes == store.records.numel()


def test_an_arena_that_is_too_small_names_the_need():
    lay = ref.layout(small_recordings(), 1)
    seen = []

    def lazily():
        for rec in small_recordings():
            seen.append(rec[0])
            yield rec
    with pytest.raises(ValueError, match=str(8 * lay['kept'])):
        HostWindowStore(lazily(), 1, (-20_000, 0), 'cpu', sensor_hw=(24, 32), capacity_bytes=8 * lay['kept'] - 8)
    assert len(seen) == 3                                                     # the scan went on to the end to know the need
    assert HostWindowStore(small_recordings(), 1, (-20_000, 0), 'cpu', sensor_hw=(24, 32), capacity_bytes=8 * lay['kept']).kept_records == lay['kept']
    # no capacity given, no device to ask: the size of the recordings bounds the arena (a list is measured, a generator needs the figure)
    assert HostWindowStore(small_recordings(), 1, (-20_000, 0), 'cpu', sensor_hw=(24, 32)).capacity_bytes >= 8 * lay['kept']
    with pytest.raises(ValueError):
        HostWindowStore(lazily(), 1, (-20_000, 0), 'cpu', sensor_hw=(24, 32))


def test_frames_refuse_another_window_or_slice_count():
    store = HostWindowStore(small_recordings(), 2, (-20_000, 0), 'cpu', sensor_hw=(24, 32), capacity_bytes=12_000)
    idx = torch.zeros(1, dtype=torch.int64)
    for kw in (dict(Tl=1, window=-20), dict(Tl=2, window=-50)):
        with pytest.raises(ValueError):
            store.frames(idx, [(32, 24, 0, 0, 0)], types.SimpleNamespace(Tm=3, input_size=(32, 48), **kw))


def test_store_records_selects_the_class():
    exp = types.SimpleNamespace(Tm=3, Tl=1, input_size=(32, 48), test_size=(32, 48), num_classes=2, window=-20, store_recordings=(2, 4, 300))
    assert type(data.gen1_store_for(exp, device='cpu')) is data.Gen1Store                              # the default is today's path
    exp.store_records = 'all'
    assert type(data.gen1_store_for(exp, device='cpu')) is data.Gen1Store
    exp.store_records = 'some'
    with pytest.raises(ValueError):
        data.gen1_store_for(exp, device='cpu')
