"""Numpy checker of the store that keeps only the records its samples read (``data.Gen1WindowStore``): the union of record ranges and
the place of every range in it (``ops.record_ranges_union``), the gather (``ops.records_gather``) and the layout of a whole store, whose
window ranges come from the oracle's restatement of the reference's reader (oracle/events_ref.py ``search_events``).  Plain loops over
sorted ranges; tests/test_cpu_window_store.py compares the union with a per-record mask."""
import numpy as np

from eas_snn_amd import data
from oracle import events_ref


def union(ranges):
    """(segments int64 [S, 2] sorted, disjoint, non-empty, touching ranges merged; seg_dst int64 [S + 1] from 0; mapped int64 [M, 2]: every
    range's place in the segments laid back to back, an empty range at (0, 0)) of the ranges int64 [M, 2]"""
    ranges = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    segments = []
    for a, e in sorted((int(a), int(e)) for a, e in ranges if e > a):
        if segments and a <= segments[-1][1]:
            segments[-1][1] = max(segments[-1][1], e)
        else:
            segments.append([a, e])
    segments = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
    seg_dst = np.r_[0, np.cumsum(segments[:, 1] - segments[:, 0])].astype(np.int64)
    mapped = np.zeros_like(ranges)
    for i, (a, e) in enumerate(ranges):
        if e > a:
            j = int(np.searchsorted(segments[:, 0], a, side='right')) - 1
            assert segments[j, 0] <= a and e <= segments[j, 1]
            mapped[i] = seg_dst[j] + a - segments[j, 0], seg_dst[j] + e - segments[j, 0]
    return segments, seg_dst, mapped


def gather(src, segments, seg_dst, dst, dst_offset=0):
    """``dst`` (records as rows) with the segments of ``src`` copied in from row ``dst_offset`` on; a copy is returned"""
    out = dst.copy()
    for (a, e), d in zip(segments, seg_dst[:-1]):
        out[dst_offset + d:dst_offset + d + e - a] = src[a:e]
    return out


def random_ranges(rng, n_records, m, max_len=None):
    """``m`` ranges over ``n_records`` records of every kind: unsorted, overlapping, nested, duplicated, touching, empty; a range holds
    ``max_len`` records at most (an eighth of all unless given; a touching one may be longer)"""
    max_len = max_len or max(n_records // 8, 2)
    out = []
    while len(out) < m:
        a = int(rng.integers(0, n_records))
        e = int(rng.integers(a + 1, min(a + max_len, n_records) + 1))
        kind = int(rng.integers(0, 6))
        out.append((a, e))
        if kind == 0:
            out.append((a, e))                                                   # a duplicate
        elif kind == 1 and e - a > 2:
            out.append((a + 1, e - 1))                                           # nested
        elif kind == 2 and e < n_records:
            out.append((e, int(rng.integers(e + 1, n_records + 1))))             # touching
        elif kind == 3:
            out.append((a, a))                                                   # empty, inside
        elif kind == 4:
            out.append((n_records, n_records))                                   # empty, at the end
    out = np.asarray(out[:m], dtype=np.int64)
    return out[rng.permutation(len(out))]


# ------------------------------------------------------------------------------------------------ the recordings of the store tests
WINDOW, SENSOR = (-20_000, 0), (240, 304)


def _recording(name, t, times, seed):
    rng = np.random.default_rng(seed)
    H, W = SENSOR
    x, y, p = rng.integers(0, W, len(t)), rng.integers(0, H, len(t)), rng.integers(0, 2, len(t))
    rows = [(lt, 30 + 5 * k, 20 + 3 * k, 60, 50 + k, k % 2, 1.0, 0) for k, lt in enumerate(times)]
    if len(times):
        rows.append((times[-1], 100, 80, 70, 60, 1, 1.0, 1))                     # the last label group holds two boxes
    return name, data.encode_dat(t, x, y, p, H, W), np.array(rows, dtype=data.GEN1_BBOX_DTYPE)


def recordings():
    """three seeded recordings of 20 000 events and 6 labels 50 ms apart, and between them: one of 250 000 events (the reader's bisection
    probes; one label whose window start IS the first probe), one with gaps in its events (a window that steps back and finds events, one
    that stays empty), one without labels, one without events"""
    plain = data.synth_gen1_recordings(3, 6, 20_000, label_period_us=50_000)
    rng = np.random.default_rng(77)
    t_big = np.sort(rng.integers(1_000_000, 1_400_000, 250_000))
    probe = int(t_big[125_000]) - WINDOW[0]                                      # the label whose window starts at the probed record's time
    big = _recording('big', t_big, sorted([1_050_000, 1_100_000, 1_150_000, probe, 1_300_000, 1_350_000]), 78)
    t_gap = np.sort(np.concatenate([rng.integers(1_000_000, 1_100_000, 4000), rng.integers(1_300_000, 1_400_000, 4000)]))
    gap = _recording('gap', t_gap, [1_050_000, 1_125_000, 1_250_000, 1_350_000], 79)
    nolabels = _recording('nolabels', np.sort(rng.integers(1_000_000, 1_200_000, 5000)), [], 80)
    noevents = _recording('noevents', np.zeros(0, dtype=np.int64), [1_050_000, 1_100_000], 81)
    return [plain[0], big, gap, plain[1], nolabels, noevents, plain[2]]


def record_times(dat):
    start = data.parse_dat_header(dat)[0]
    return np.ascontiguousarray(dat[start:]).view('<u4').reshape(-1, 2)[:, 0].astype(np.int64)


def layout(recs, Tl, window=WINDOW):
    """what the store keeps of the recordings: ``total`` and ``kept`` records, ``file_offsets`` of the kept areas, ``full_ranges`` int64
    [G, Tl, 2] into all records back to back (what ``Gen1Store.frames`` searches), ``sample_ranges`` int64 [G, Tl, 2] into the kept ones,
    and ``keep``: the indices of the kept records among all"""
    step = window[1] - window[0]
    total, offsets, full, mapped_all, keep = 0, [0], [], [], []
    for _, dat, rows in recs:
        t = record_times(dat)
        times = np.unique(rows['t'].astype(np.int64))
        local = np.array([events_ref.search_events(t, int(lt) + k * step, window, Tl) for lt in times for k in range(-Tl + 1, 1)],
                         dtype=np.int64).reshape(-1, 2)
        segments, seg_dst, mapped = union(local)
        full.append(local + total)
        mapped_all.append(mapped + offsets[-1])
        keep += [np.arange(a, e) + total for a, e in segments]
        offsets.append(offsets[-1] + int(seg_dst[-1]))
        total += len(t)
    cat = lambda parts: np.concatenate(parts).reshape(-1, Tl, 2)               # noqa: E731
    return dict(total=total, kept=offsets[-1], file_offsets=np.asarray(offsets, dtype=np.int64), full_ranges=cat(full),
                sample_ranges=cat(mapped_all), keep=np.concatenate(keep) if keep else np.zeros(0, dtype=np.int64))
