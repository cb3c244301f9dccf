"""Plain numpy checker of the N-Caltech101 front end with measure 'timesurface' (eas_event_timesurface_atis, eas_frames_letterbox_f64),
written from the definition: an event of time t in a macro slice whose last member event has time t_target adds
``1 - tanh((t_target - t) / tau)`` to its bin, in event order, in float64 (NCaltech.get_measure_func / agrregate, ncaltech.py:218-237;
event_reps.py:13-19).  The decode is tests/ncaltech_ref.py's; the slicing is its rule walked once more with the event's time kept, and every
call checks the walk against ``ncaltech_ref.atis_frames``.  tests/test_cpu_ncaltech_ts.py pins ``atis_timesurface_frames`` to
tests/golden/ncaltech_timesurface.npz, recorded from the reference (scripts/gen_golden_ncaltech_ts.py).  The linear resize restates
``linear_tap`` of csrc/count_resize.h (OpenCV's INTER_LINEAR for float64 images; parity against cv2 unpinned, no cv2 here)."""
import numpy as np

import ncaltech_ref
from ncaltech_ref import decode_atis

ONE = 2 ** 48               # a weight of 1 in the kernel's 64-bit bins
CAPACITY = (2 ** 64 - 1) // ONE


COUNT_CASES = ['plain_1x4', 'window0_2x3', 'negwin_1x8', 'negwin_hi_2x3', 'overflow_1x4', 'overflow_negwin_2x3', 'overflow_1x8', 'short_span_w0',
               'polarity_1x4', 'polarity_2x3']
HOT = 'hot_pixel_1x4'
CASES = COUNT_CASES + [HOT]


CANVAS = (64, 64)
# (nw, nh, dx, dy, flip) on the 64 x 64 canvas for the 36 x 48 sensor: the letterbox (scale 4/3) pasted 8 rows down, a shrunk and mirrored
# frame at an offset, the identity size at an offset
PARAMS = [(64, 48, 0, 8, 0), (40, 30, 11, 9, 1), (48, 36, 5, 3, 0)]


def case_params(n):
    """int32 [n, 5]: recording b takes PARAMS[b % 3]"""
    return np.array([PARAMS[b % len(PARAMS)] for b in range(n)], np.int32)


def load_cases():
    """{case: dict(bufs, window, Tl, Tm, H, W, frames float64 [B, Tl, Tm, 2, H, W])}: the recordings of tests/golden/ncaltech_atis.npz with
    the time-surface frames of tests/golden/ncaltech_timesurface.npz, and the hot-pixel recording that file brings itself"""
    from conftest import load_golden, split_cases
    inputs, ts = split_cases(load_golden('ncaltech_atis')), split_cases(load_golden('ncaltech_timesurface'))
    assert sorted(ts) == sorted(CASES)
    cases = {}
    for name in CASES:
        src = ts[name] if name == HOT else inputs[name]
        off = src['offsets']
        cases[name] = dict(bufs=[src['bytes'][5 * off[b]:5 * off[b + 1]] for b in range(len(off) - 1)],
                           window=tuple(int(v) for v in src['window']) if int(src['has_window']) else None,
                           Tl=int(src['Tl']), Tm=int(src['Tm']), H=int(src['H']), W=int(src['W']), frames=ts[name]['frames'])
    cases[HOT]['counts'] = ts[HOT]['counts']
    return cases


def atis_timesurface_frames(buf, window, Tl, Tm, H, W, tau=500e3, quantised=False):
    """-> (frames float64 [Tl, Tm, 2, H, W], counts int32 of the same shape, oob, flags) of one recording.  ``quantised``: the kernel's
    arithmetic -- every weight rounded to a multiple of 2^-48, the integer sum of a bin converted once"""
    frames = np.zeros((Tl, Tm, 2, H, W), dtype=np.float64)
    bins = np.zeros((Tl, Tm, 2, H, W), dtype=object) if quantised else None
    counts = np.zeros((Tl, Tm, 2, H, W), dtype=np.int32)
    want_counts, want_oob, want_flags = ncaltech_ref.atis_frames(buf, window, Tl, Tm, H, W)
    t, x, y, p = decode_atis(buf)
    if len(t) and window is not None and window[0] < 0:
        keep = (t > t[-1] + window[0]) & (t <= t[-1] + window[1])
        t, x, y, p = t[keep], x[keep], y[keep], p[keep]
    oob = 0
    if len(t):
        t0 = int(t[0])
        mw = (int(t[-1]) - t0) // Tl
        for k in range(Tl):
            m = (t >= t0 + k * mw) & (t < t0 + (k + 1) * mw)
            if not m.any():
                continue
            tk, xk, yk, pk = t[m], x[m], y[m], p[m]
            f, t_target = int(tk[0]), int(tk[-1])
            w = (t_target - f) // Tm
            if w <= 0:
                continue
            weight = 1 - np.tanh((t_target - tk) / tau)                 # the reference's expression on the slice's int64 times
            for tt, xx, yy, pp, ww in zip(tk.tolist(), xk.tolist(), yk.tolist(), pk.tolist(), weight.tolist()):
                q = (tt - f) // w
                if q < 0 or q >= Tm:
                    continue
                if xx >= W or yy >= H:
                    oob += 1
                    continue
                at = (k, q, 1 if pp else 0, yy, xx)
                counts[at] += 1
                if quantised:
                    bins[at] += int(np.rint(ww * ONE))
                else:
                    frames[at] += ww
    assert np.array_equal(counts, want_counts) and oob == want_oob, 'the walk is not the slicing of ncaltech_ref.atis_frames'
    if quantised:
        frames = (bins.astype(np.float64) / ONE).reshape(frames.shape)   # int -> float64 rounds to nearest even, the division is exact
    return frames, counts, oob, want_flags


def linear_taps(n_src, n_dst):
    """-> (index int64 [n_dst, 2], weights float32 [n_dst, 2]) of one axis: ``linear_tap``"""
    j = np.arange(n_dst, dtype=np.float64)
    f = ((j + 0.5) * (np.float64(n_src) / np.float64(n_dst)) - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= n_src - 1
    f[low | high] = 0
    s = np.where(low, 0, np.where(high, n_src - 1, s))
    idx = np.stack([s, np.minimum(s + 1, n_src - 1)], axis=1)
    c = np.stack([np.float32(1) - f, f], axis=1)
    assert c.dtype == np.float32
    return idx, c


def resize_linear(img, nw, nh):
    """[..., H, W] -> float64 [..., nh, nw]: horizontal pass first, float64 products added left to right; the identity size is a copy"""
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[-2:]
    if nw == W and nh == H:
        return img.copy()
    ix, cx = linear_taps(W, nw)
    iy, cy = linear_taps(H, nh)
    cx, cy = cx.astype(np.float64), cy.astype(np.float64)
    h = img[..., :, ix[:, 0]] * cx[:, 0] + img[..., :, ix[:, 1]] * cx[:, 1]
    return h[..., iy[:, 0], :] * cy[:, 0, None] + h[..., iy[:, 1], :] * cy[:, 1, None]


def letterbox(frames, params, h, w, interp):
    """frames [B, ..., H, W], params rows (nw, nh, dx, dy, flip) with the paste rectangle on the canvas -> float64 [B, ..., h, w]"""
    if interp == 'cubic':
        return ncaltech_ref.letterbox_cubic(frames, params, h, w)
    assert interp == 'linear'
    frames = np.asarray(frames)
    out = np.zeros(frames.shape[:-2] + (h, w), dtype=np.float64)
    for b, (nw, nh, dx, dy, flip) in enumerate(np.asarray(params).reshape(-1, 5).tolist()):
        out[b, ..., dy:dy + nh, dx:dx + nw] = resize_linear(frames[b], nw, nh)
        if flip:
            out[b] = out[b, ..., ::-1]
    return out
