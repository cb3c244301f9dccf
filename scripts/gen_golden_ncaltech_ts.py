"""Writes tests/golden/ncaltech_timesurface.npz: the float64 frames the REFERENCE's own ``NCaltech.read_ATIS``, ``generate_slices`` and
``agrregate('micro_sum')`` make with ``measure='timesurface'`` (get_measure_func: ``timesurface_measure(tau=500e3, decay='tanh')``, t_target =
the time of the macro slice's last event) of the recordings of tests/golden/ncaltech_atis.npz, plus one hot-pixel recording of its own.

    python scripts/gen_golden_ncaltech_ts.py --reference /path/to/EAS-SNN [--out tests/golden/ncaltech_timesurface.npz]

A sibling of scripts/gen_golden_ncaltech.py, whose loader, record writer and case list it imports: that script and its fixture stay as they
are.  Only data is stored.  For the cases of the count fixture only ``<case>/frames`` float64 [B, Tl, Tm, 2, H, W] (their ``bytes``,
``offsets``, ``window``, ``Tl``, ``Tm`` are read from ncaltech_atis.npz: the case list is regenerated here from the same seed and checked
against that file).  For ``hot_pixel_1x4`` every field of the count fixture, and ``counts`` int32: the reference's frames of the same recording
with measure 'count'."""
import argparse
import io
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_golden_ncaltech import H, W, load_reference, make_cases, records      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOT = 'hot_pixel_1x4'


def run_reference(NCaltech, buf, window, Tl, Tm, measure):
    ns = types.SimpleNamespace(dtype=np.dtype([('x', int), ('y', int), ('t', int), ('p', int)]), img_size=(H, W),
                               slice_args=dict(num_slice=Tl, overlap=0, aggregation='micro_sum', micro_slice=Tm, measure=measure))
    for m in ('get_measure_func', 'generate_slices', 'agrregate'):
        setattr(ns, m, types.MethodType(getattr(NCaltech, m), ns))
    events = NCaltech.read_ATIS(ns, io.BytesIO(buf.tobytes()), window=window, is_stream=True)
    slices, _ = NCaltech.generate_slices(ns, events, ns.slice_args['num_slice'], ns.slice_args['overlap'])
    frames = np.stack([NCaltech.agrregate(ns, s, aggregation=ns.slice_args['aggregation'], t_target=s[-1]['t']) for s in slices], axis=0)
    assert frames.shape == (Tl, Tm, 2, H, W) and frames.dtype == np.float64
    return frames


def hot_pixel_recording():
    """1300 events over 60 ms (1307 records: six chunks of 256), 650 of the events between 18 and 29 ms -- inside micro slice 1 of 4 -- on
    pixel (p, y, x) = (1, 11, 17), overflow records in front of the recording, between the hot events and behind the last event"""
    rng = np.random.default_rng(77)
    n, at = 1300, (0, 420, 421, 600, 777, 1000, 1300)
    t = np.sort(np.concatenate([rng.integers(0, 60_000, n - 700), rng.integers(18_000, 29_000, 700)])) + 8192 * len(at)
    t[0], t[n - 3:] = 8192 * len(at), t[-1]
    x, y, p = rng.integers(0, W, n), rng.integers(0, H, n), (rng.random(n) < 0.5).astype(np.int64)
    inside = np.flatnonzero((t >= t[0] + 18_000) & (t < t[0] + 29_000))
    hot = rng.choice(inside, 650, replace=False)
    x[hot], y[hot], p[hot] = 17, 11, 1
    assert (np.sort(hot) < 420).any() and (np.sort(hot) > 777).any(), 'overflow records stand between the hot events'
    return records(t, x, y, p, overflow_at=at, overflow_raw=int(rng.integers(0, 1 << 23)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of an EAS-SNN checkout (holds yolox/data/datasets/ncaltech.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'ncaltech_timesurface.npz'))
    args = ap.parse_args()
    NCaltech = load_reference(args.reference)
    count_fixture = np.load(os.path.join(ROOT, 'tests', 'golden', 'ncaltech_atis.npz'))
    out = {}
    for name, c in make_cases().items():
        assert np.array_equal(np.concatenate(c['bufs']), count_fixture[f'{name}/bytes']), f'{name}: not the recordings of ncaltech_atis.npz'
        frames = np.stack([run_reference(NCaltech, b, c['window'], c['Tl'], c['Tm'], 'timesurface') for b in c['bufs']])
        counts = count_fixture[f'{name}/frames']
        assert np.array_equal(frames == 0, counts == 0) and (frames <= counts).all()
        out[f'{name}/frames'] = frames
        print(f'{name}: weight sum {frames.sum():.6f} of {int(counts.sum())} events')
    buf = hot_pixel_recording()
    Tl, Tm = 1, 4
    frames = run_reference(NCaltech, buf, None, Tl, Tm, 'timesurface')[None]
    counts = run_reference(NCaltech, buf, None, Tl, Tm, 'count')[None]
    assert np.array_equal(counts, counts.astype(np.int32)) and counts.max() >= 600 and np.array_equal(frames == 0, counts == 0)
    assert len(buf) // 5 > 4 * 256 and counts[0, 0, 1, 1, 11, 17] == counts.max()
    out[f'{HOT}/bytes'] = buf
    out[f'{HOT}/offsets'] = np.asarray([0, len(buf) // 5], np.int64)
    out[f'{HOT}/has_window'], out[f'{HOT}/window'] = np.int64(0), np.zeros(2, np.int64)
    out[f'{HOT}/Tl'], out[f'{HOT}/Tm'], out[f'{HOT}/H'], out[f'{HOT}/W'] = np.int64(Tl), np.int64(Tm), np.int64(H), np.int64(W)
    out[f'{HOT}/frames'] = frames
    out[f'{HOT}/counts'] = counts.astype(np.int32)
    print(f'{HOT}: {len(buf) // 5} records, {int(counts.sum())} events binned, {int(counts.max())} in the hot bin, weight sum {frames.sum():.6f}')
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
