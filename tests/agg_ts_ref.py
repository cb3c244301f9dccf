"""Plain numpy checker of the N-Caltech101 front end with aggregation 'timesurface' (eas_event_latest_surface_atis), written from the
definition (NCaltech.agrregate 'timesurface', ncaltech.py:255-257; to_timesurface_numpy, event_reps.py:141-160): per macro slice a memory
[2, H, W] of integer zeros takes the time of every event of micro slice q -- a running ``np.maximum.at``: times ascend, so the reference's
last write is the maximum, and the memory is not cleared between micro slices -- and frame q is
``exp(-((q + 1) * w + f - memory) / tau)`` in float64, f the macro slice's first time, w its micro window.  The decode is
tests/ncaltech_ref.py's, the slicing its rule walked once more, and every call checks the walk against ``ncaltech_ref.atis_frames``.
tests/test_cpu_agg_timesurface.py pins ``atis_latest_surface`` to tests/golden/ncaltech_agg_timesurface.npz, recorded from the reference
(scripts/gen_golden_ncaltech_aggts.py).  The resize rules are ``ncaltech_ts_ref.letterbox``."""
import numpy as np

import ncaltech_ref
from ncaltech_ref import decode_atis

WINDOW0 = 8                 # flag bit 3: a macro slice holds events and has micro window 0 (the reference raises IndexError)
HOT = 'hot_every_slice_1x4'
HOT_PIXEL = (1, 11, 17)     # (p, y, x)
CASES = ['plain_1x4', 'window0_2x3', 'negwin_1x8', 'negwin_hi_2x3', 'overflow_1x4', 'overflow_negwin_2x3', 'overflow_1x8', 'short_span_w0',
         'polarity_1x4', 'polarity_2x3', HOT]


def load_cases():
    """{case: dict(bufs, window, Tl, Tm, H, W, frames float64 [B, Tl, Tm, 2, H, W], raises int64 [B])}"""
    from conftest import load_golden, split_cases
    fixture = split_cases(load_golden('ncaltech_agg_timesurface'))
    assert sorted(fixture) == sorted(CASES)
    cases = {}
    for name in CASES:
        src = fixture[name]
        off = src['offsets']
        cases[name] = dict(bufs=[src['bytes'][5 * off[b]:5 * off[b + 1]] for b in range(len(off) - 1)],
                           window=tuple(int(v) for v in src['window']) if int(src['has_window']) else None,
                           Tl=int(src['Tl']), Tm=int(src['Tm']), H=int(src['H']), W=int(src['W']), frames=src['frames'], raises=src['raises'])
    return cases


def atis_latest_surface(buf, window, Tl, Tm, H, W, tau=10e3):
    """-> (frames float64 [Tl, Tm, 2, H, W], oob, flags) of one recording; flags: bits 0 and 1 of ``ncaltech_ref.atis_frames`` and WINDOW0.
    The frames of a macro slice that is empty or has micro window 0 are zero."""
    frames = np.zeros((Tl, Tm, 2, H, W), dtype=np.float64)
    counts, oob, flags = ncaltech_ref.atis_frames(buf, window, Tl, Tm, H, W)
    t, x, y, p = decode_atis(buf)
    if len(t) and window is not None and window[0] < 0:
        keep = (t > t[-1] + window[0]) & (t <= t[-1] + window[1])
        t, x, y, p = t[keep], x[keep], y[keep], p[keep]
    if len(t):
        t0 = int(t[0])
        mw = (int(t[-1]) - t0) // Tl
        for k in range(Tl):
            m = (t >= t0 + k * mw) & (t < t0 + (k + 1) * mw)
            if not m.any():
                continue
            tk, xk, yk, pk = t[m], x[m], y[m], p[m]
            f = int(tk[0])
            w = (int(tk[-1]) - f) // Tm
            if w <= 0:
                flags |= WINDOW0
                continue
            memory = np.zeros((2, H, W), dtype=np.int64)
            for q in range(Tm):
                s = (tk >= f + q * w) & (tk < f + (q + 1) * w) & (xk < W) & (yk < H)
                at = ((pk[s] != 0).astype(np.int64), yk[s], xk[s])
                hit = np.zeros((2, H, W), dtype=bool)
                hit[at] = True
                assert np.array_equal(hit, counts[k, q] > 0), 'the walk is not the slicing of ncaltech_ref.atis_frames'
                np.maximum.at(memory, at, tk[s])
                frames[k, q] = np.exp(-((q + 1) * w + f - memory) / tau)
    return frames, oob, flags


def exponent_ticks(frames, tau=10e3):
    """rint(log(frames) * tau): the integer latest - end of the micro slice that a surface encodes (frames > 0)"""
    return np.rint(np.log(frames) * tau)
