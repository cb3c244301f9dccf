"""Writes tests/golden/ncaltech_atis.npz: byte images of small ATIS recordings and the count frames the REFERENCE's own
``NCaltech.read_ATIS``, ``generate_slices`` and ``agrregate('micro_sum')`` (measure 'count', overlap 0) make of them.

    python scripts/gen_golden_ncaltech.py --reference /path/to/EAS-SNN [--out tests/golden/ncaltech_atis.npz]

yolox/data/datasets/ncaltech.py is loaded by file location under its package name, next to the real yolox/utils/event_reps.py and
yolox/utils/util.py (``make_structured_array``); everything else it imports (cv2, loguru, pycocotools.coco, ..dataloading,
.datasets_wrapper, yolox.utils.boxes) is an empty stand-in.  The methods run unbound on a ``SimpleNamespace(dtype, img_size, slice_args)``
exactly as ``NCaltech.__getitem__`` chains them (ncaltech.py:178-183), ``read_ATIS(..., is_stream=True)`` on a ``BytesIO``.  No bytecode is
written into the reference tree.  Only data is stored, per case: ``bytes`` uint8, ``offsets`` int64 (records), ``window`` int64 [2]
(``has_window`` 0: None was passed), ``Tl``, ``Tm``, ``H``, ``W`` and ``frames`` int32 [B, Tl, Tm, 2, H, W]."""
import argparse
import importlib.util
import io
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True

H, W = 36, 48


class _Stub(types.ModuleType):
    """an empty module: every name it is asked for is a do-nothing class"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        cls = type(name, (), {'mosaic_getitem': staticmethod(lambda fn: fn)})
        setattr(self, name, cls)
        return cls


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(root):
    for name in ('cv2', 'loguru', 'pycocotools', 'pycocotools.coco', 'yolox', 'yolox.data', 'yolox.data.datasets', 'yolox.data.dataloading',
                 'yolox.data.datasets.datasets_wrapper', 'yolox.utils', 'yolox.utils.boxes'):
        sys.modules[name] = _Stub(name)
    try:
        import PIL  # noqa: F401
    except ImportError:
        sys.modules['PIL'] = _Stub('PIL')
    _load('yolox.utils.util', os.path.join(root, 'yolox', 'utils', 'util.py'))
    _load('yolox.utils.event_reps', os.path.join(root, 'yolox', 'utils', 'event_reps.py'))
    return _load('yolox.data.datasets.ncaltech', os.path.join(root, 'yolox', 'data', 'datasets', 'ncaltech.py')).NCaltech


def run_reference(NCaltech, buf, window, Tl, Tm):
    ns = types.SimpleNamespace(dtype=np.dtype([('x', int), ('y', int), ('t', int), ('p', int)]), img_size=(H, W),
                               slice_args=dict(num_slice=Tl, overlap=0, aggregation='micro_sum', micro_slice=Tm, measure='count'))
    for m in ('get_measure_func', 'generate_slices', 'agrregate'):
        setattr(ns, m, types.MethodType(getattr(NCaltech, m), ns))
    events = NCaltech.read_ATIS(ns, io.BytesIO(buf.tobytes()), window=window, is_stream=True)
    slices, _ = NCaltech.generate_slices(ns, events, ns.slice_args['num_slice'], ns.slice_args['overlap'])
    frames = np.stack([NCaltech.agrregate(ns, s, aggregation=ns.slice_args['aggregation'], t_target=s[-1]['t']) for s in slices], axis=0)
    assert frames.shape == (Tl, Tm, 2, H, W) and np.array_equal(frames, frames.astype(np.int32))
    return frames.astype(np.int32)


def records(t, x, y, p, overflow_at=(), overflow_raw=0):
    """byte image: the events with DECODED times t, an overflow record in front of event index i for every i of overflow_at (len(t): behind
    the last event); the overflow records carry ``overflow_raw`` in their time field and stray x / p bits"""
    t = np.asarray(t, np.int64)
    n, ov = len(t), np.sort(np.asarray(list(overflow_at), np.int64))
    nb = np.searchsorted(ov, np.arange(n), side='right')
    raw = t - 8192 * nb
    assert ((raw >= 0) & (raw < 1 << 23)).all()
    rec = np.zeros((n + len(ov), 5), np.uint8)
    pos = np.arange(n) + nb
    rec[:, 0], rec[:, 1] = 7, 240
    rec[:, 2], rec[:, 3], rec[:, 4] = 128 | ((overflow_raw >> 16) & 127), (overflow_raw >> 8) & 255, overflow_raw & 255
    rec[pos, 0], rec[pos, 1] = x, y
    rec[pos, 2] = (np.asarray(p, np.int64) << 7) | (raw >> 16)
    rec[pos, 3], rec[pos, 4] = (raw >> 8) & 255, raw & 255
    return rec.reshape(-1)


def stream(rng, n, span, t_first=0, last_ties=1, p_one=0.5):
    """n events, sorted times over ``span`` us from t_first, the last ``last_ties`` of them on the last timestamp"""
    t = np.sort(rng.integers(t_first, t_first + span, size=n))
    t[n - last_ties:] = t[-1]
    return t, rng.integers(0, W, n), rng.integers(0, H, n), (rng.random(n) < p_one).astype(np.int64)


def make_cases():
    rng = np.random.default_rng(2024)
    cases = {}

    def add(name, bufs, window, Tl, Tm):
        cases[name] = dict(bufs=bufs, window=window, Tl=Tl, Tm=Tm)

    add('plain_1x4', [records(*stream(rng, n, 50_000, 1000, ties)) for n, ties in ((700, 5), (1500, 1), (90, 3))], None, 1, 4)
    add('window0_2x3', [records(*stream(rng, n, 80_000, 0, ties)) for n, ties in ((900, 4), (333, 2))], (0, 0), 2, 3)
    add('negwin_1x8', [records(*stream(rng, n, 60_000, 500, ties)) for n, ties in ((1200, 6), (800, 1))], (-20_000, 0), 1, 8)
    add('negwin_hi_2x3', [records(*stream(rng, n, 90_000, 0, ties)) for n, ties in ((1000, 3), (1100, 1))], (-30_000, -5_000), 2, 3)
    ov = []
    for n, at in ((1000, (0, 400, 401, 1000)), (600, (0, 0, 300)), (500, (250, 500, 500))):
        t, x, y, p = stream(rng, n, 70_000, 8192 * len(at), 4)
        ov.append(records(t, x, y, p, overflow_at=at, overflow_raw=int(rng.integers(0, 1 << 23))))
    add('overflow_1x4', ov, None, 1, 4)
    add('overflow_negwin_2x3', ov, (-40_000, 0), 2, 3)
    add('overflow_1x8', ov[:2], (0, 0), 1, 8)
    t = np.array([100, 100, 101, 101, 101, 102, 102, 103, 103, 103, 103, 103])
    add('short_span_w0', [records(t, rng.integers(0, W, 12), rng.integers(0, H, 12), rng.integers(0, 2, 12)),
                          records(t * 3, rng.integers(0, W, 12), rng.integers(0, H, 12), rng.integers(0, 2, 12))], None, 1, 4)
    add('polarity_1x4', [records(*stream(rng, 800, 40_000, 0, 2, p_one=0.9)), records(*stream(rng, 800, 40_000, 0, 2, p_one=0.05))], None, 1, 4)
    add('polarity_2x3', [records(*stream(rng, 900, 40_000, 0, 1, p_one=0.95))], (-25_000, 0), 2, 3)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of an EAS-SNN checkout (holds yolox/data/datasets/ncaltech.py)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden',
                                                  'ncaltech_atis.npz'))
    args = ap.parse_args()
    NCaltech = load_reference(args.reference)
    out = {}
    for name, c in make_cases().items():
        frames = np.stack([run_reference(NCaltech, b, c['window'], c['Tl'], c['Tm']) for b in c['bufs']])
        out[f'{name}/bytes'] = np.concatenate(c['bufs'])
        out[f'{name}/offsets'] = np.cumsum([0] + [len(b) // 5 for b in c['bufs']]).astype(np.int64)
        out[f'{name}/has_window'] = np.int64(c['window'] is not None)
        out[f'{name}/window'] = np.asarray(c['window'] if c['window'] is not None else (0, 0), np.int64)
        for k in ('Tl', 'Tm'):
            out[f'{name}/{k}'] = np.int64(c[k])
        out[f'{name}/H'], out[f'{name}/W'] = np.int64(H), np.int64(W)
        out[f'{name}/frames'] = frames
        print(f'{name}: {len(c["bufs"])} recordings, {len(out[f"{name}/bytes"]) // 5} records, {int(frames.sum())} events binned, '
              f'{int((frames.reshape(len(c["bufs"]), -1).sum(1) == 0).sum())} recordings all zero')
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
