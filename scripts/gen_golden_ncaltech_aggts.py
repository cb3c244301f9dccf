"""Writes tests/golden/ncaltech_agg_timesurface.npz: the float64 frames the REFERENCE's own ``NCaltech.read_ATIS``, ``generate_slices`` and
``agrregate(aggregation='timesurface')`` (per macro slice: ``generate_slices(events, Tm, overlap=0)`` and ``to_timesurface_numpy(dt = the
micro window, tau=10e3)``, ncaltech.py:178-183, 255-257; event_reps.py:141-160) make of the recordings of
scripts/gen_golden_ncaltech.make_cases(), plus one recording of its own with overflow records and a pixel hit in every micro slice.

    python scripts/gen_golden_ncaltech_aggts.py --reference /path/to/EAS-SNN [--out tests/golden/ncaltech_agg_timesurface.npz]

A sibling of scripts/gen_golden_ncaltech.py, whose loader, record writer and case list it imports.  Only data is stored, per case: ``bytes``
uint8, ``offsets`` int64 (records), ``window`` int64 [2] (``has_window`` 0: None was passed), ``Tl``, ``Tm``, ``H``, ``W``, ``frames`` float64
[B, Tl, Tm, 2, H, W] and ``raises`` int64 [B]: 1 for a recording on which the reference raised (a micro window of 0: ``slices[0][0]`` of an
empty slice, IndexError), its frames stored as zeros.  No bytecode is written into the reference tree."""
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
HOT = 'hot_every_slice_1x4'
HOT_PIXEL = (1, 11, 17)             # (p, y, x)


def run_reference(NCaltech, buf, window, Tl, Tm):
    """-> (frames float64 [Tl, Tm, 2, H, W], raises)"""
    ns = types.SimpleNamespace(dtype=np.dtype([('x', int), ('y', int), ('t', int), ('p', int)]), img_size=(H, W),
                               slice_args=dict(num_slice=Tl, overlap=0, aggregation='timesurface', micro_slice=Tm, measure='count'))
    for m in ('get_measure_func', 'generate_slices', 'agrregate'):
        setattr(ns, m, types.MethodType(getattr(NCaltech, m), ns))
    events = NCaltech.read_ATIS(ns, io.BytesIO(buf.tobytes()), window=window, is_stream=True)
    slices, _ = NCaltech.generate_slices(ns, events, ns.slice_args['num_slice'], ns.slice_args['overlap'])
    try:
        frames = np.stack([NCaltech.agrregate(ns, s, aggregation=ns.slice_args['aggregation'], t_target=s[-1]['t']) for s in slices], axis=0)
    except IndexError:
        return np.zeros((Tl, Tm, 2, H, W)), 1
    assert frames.shape == (Tl, Tm, 2, H, W) and frames.dtype == np.float64
    return frames, 0


def hot_every_slice_recording():
    """900 events over 48 ms, overflow records in front of the recording, between the events and behind the last one; pixel HOT_PIXEL is hit
    four times in every quarter of the span (micro slices of Tm = 4), and once more by the very first event"""
    rng = np.random.default_rng(91)
    n, at = 900, (0, 300, 301, 640, 900)
    t = np.sort(rng.integers(0, 48_000, n)) + 8192 * len(at)
    t[0], t[n - 2:] = 8192 * len(at), t[-1]
    x, y, p = rng.integers(0, W, n), rng.integers(0, H, n), (rng.random(n) < 0.5).astype(np.int64)
    hot = [0]
    for q in range(4):
        inside = np.flatnonzero((t >= t[0] + 12_000 * q + 500) & (t < t[0] + 12_000 * (q + 1) - 500))
        hot += rng.choice(inside, 4, replace=False).tolist()
    p[hot], y[hot], x[hot] = HOT_PIXEL
    return records(t, x, y, p, overflow_at=at, overflow_raw=int(rng.integers(0, 1 << 23)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of an EAS-SNN checkout (holds yolox/data/datasets/ncaltech.py)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'ncaltech_agg_timesurface.npz'))
    args = ap.parse_args()
    NCaltech = load_reference(args.reference)
    cases = make_cases()
    cases[HOT] = dict(bufs=[hot_every_slice_recording()], window=None, Tl=1, Tm=4)
    out, raised = {}, []
    for name, c in cases.items():
        runs = [run_reference(NCaltech, b, c['window'], c['Tl'], c['Tm']) for b in c['bufs']]
        frames, raises = np.stack([r[0] for r in runs]), np.asarray([r[1] for r in runs], np.int64)
        for b in np.flatnonzero(raises == 0):
            assert (frames[b] > 0).all() and (np.log(frames[b]) >= -100).all(), f'{name}[{b}]: an exponent below -100'
        assert not frames[raises == 1].any()
        raised += [f'{name}[{b}]' for b in np.flatnonzero(raises)]
        out[f'{name}/bytes'] = np.concatenate(c['bufs'])
        out[f'{name}/offsets'] = np.cumsum([0] + [len(b) // 5 for b in c['bufs']]).astype(np.int64)
        out[f'{name}/has_window'] = np.int64(c['window'] is not None)
        out[f'{name}/window'] = np.asarray(c['window'] if c['window'] is not None else (0, 0), np.int64)
        out[f'{name}/Tl'], out[f'{name}/Tm'], out[f'{name}/H'], out[f'{name}/W'] = np.int64(c['Tl']), np.int64(c['Tm']), np.int64(H), np.int64(W)
        out[f'{name}/frames'], out[f'{name}/raises'] = frames, raises
        ok = frames[raises == 0]
        print(f'{name}: {len(c["bufs"])} recordings, {int(raises.sum())} raised, values {ok.min():.3e} .. {ok.max():.6f}, '
              f'least exponent {np.log(ok.min()):.2f}' if ok.size else f'{name}: all raised')
    assert raised == ['short_span_w0[0]'], raised          # exactly the recording whose micro window is 0
    p, y, x = HOT_PIXEL
    exponent = np.rint(np.log(out[f'{HOT}/frames'][0, 0]) * 10e3)          # latest - end of the micro slice, [4, 2, H, W]
    w = -np.diff(exponent.reshape(4, -1).min(axis=1))                      # a pixel nothing touches decays by the micro window
    assert (w == w[0]).all() and w[0] > 0 and (np.diff(exponent[:, p, y, x]) > -w).all(), 'the hot pixel is hit anew in every micro slice'
    assert (out[f'{HOT}/bytes'].reshape(-1, 5)[:, 1] == 240).sum() == 5
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
