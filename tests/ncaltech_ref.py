"""Plain numpy checker of the N-Caltech101 front end (eas_event_histogram_atis, eas_counts_letterbox_ex interp = 1): the rules of
include/eas_hip.h written out event by event.  tests/test_cpu_ncaltech.py pins ``atis_frames`` to tests/golden/ncaltech_atis.npz, which
was recorded from the reference's own NCaltech.read_ATIS / generate_slices / agrregate (scripts/gen_golden_ncaltech.py).  The resize is
restated from OpenCV's published INTER_CUBIC algorithm; parity against cv2 unpinned (no cv2 here)."""
import numpy as np

OVERFLOW_Y = 240
TIME_INCREMENT = 2 ** 13


def decode_atis(buf):
    """byte image of one recording -> (t, x, y, p) int64 of its events (overflow records removed, their increments applied)"""
    raw = np.asarray(buf, dtype=np.uint8).reshape(-1, 5).astype(np.int64)
    x, y, p = raw[:, 0], raw[:, 1], raw[:, 2] >> 7
    t = ((raw[:, 2] & 127) << 16) | (raw[:, 3] << 8) | raw[:, 4]
    t = t + TIME_INCREMENT * np.cumsum(y == OVERFLOW_Y)
    ev = y != OVERFLOW_Y
    return t[ev], x[ev], y[ev], p[ev]


def atis_frames(buf, window, Tl, Tm, H, W):
    """-> (counts int32 [Tl, Tm, 2, H, W], oob, flags) of one recording"""
    out = np.zeros((Tl, Tm, 2, H, W), dtype=np.int32)
    t, x, y, p = decode_atis(buf)
    flags = 1 if (np.diff(t) < 0).any() else 0
    if len(t) and window is not None and window[0] < 0:
        keep = (t > t[-1] + window[0]) & (t <= t[-1] + window[1])
        t, x, y, p = t[keep], x[keep], y[keep], p[keep]
    if len(t) == 0:
        return out, 0, flags | 2
    t0 = int(t[0])
    mw = (int(t[-1]) - t0) // Tl
    oob = 0
    for k in range(Tl):
        m = (t >= t0 + k * mw) & (t < t0 + (k + 1) * mw)
        if not m.any():
            flags |= 2
            continue
        tk, xk, yk, pk = t[m], x[m], y[m], p[m]
        f = int(tk[0])
        w = (int(tk[-1]) - f) // Tm
        if w <= 0:
            continue
        for tt, xx, yy, pp in zip(tk.tolist(), xk.tolist(), yk.tolist(), pk.tolist()):
            q = (tt - f) // w
            if q < 0 or q >= Tm:
                continue
            if xx >= W or yy >= H:
                oob += 1
                continue
            out[k, q, 1 if pp else 0, yy, xx] += 1
    return out, oob, flags


def cubic_taps(n_src, n_dst):
    """-> (index int64 [n_dst, 4] clamped to the image, weights float32 [n_dst, 4]) of one axis"""
    j = np.arange(n_dst, dtype=np.float64)
    f = ((j + 0.5) * (np.float64(n_src) / np.float64(n_dst)) - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    one, A = np.float32(1), np.float32(-0.75)
    f1, g = f + one, one - f
    c0 = ((A * f1 - np.float32(5) * A) * f1 + np.float32(8) * A) * f1 - np.float32(4) * A
    c1 = ((A + np.float32(2)) * f - (A + np.float32(3))) * f * f + one
    c2 = ((A + np.float32(2)) * g - (A + np.float32(3))) * g * g + one
    c3 = one - c0 - c1 - c2
    c = np.stack([c0, c1, c2, c3], axis=1)
    assert c.dtype == np.float32
    idx = np.clip(s.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_src - 1)
    return idx, c


def resize_cubic(img, nw, nh):
    """[..., H, W] -> float64 [..., nh, nw]: horizontal pass first, float64 sums added left to right; the identity size is a copy"""
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[-2:]
    if nw == W and nh == H:
        return img.copy()
    ix, cx = cubic_taps(W, nw)
    iy, cy = cubic_taps(H, nh)
    cx, cy = cx.astype(np.float64), cy.astype(np.float64)
    h = img[..., :, ix[:, 0]] * cx[:, 0]
    for k in range(1, 4):
        h = h + img[..., :, ix[:, k]] * cx[:, k]
    v = h[..., iy[:, 0], :] * cy[:, 0, None]
    for k in range(1, 4):
        v = v + h[..., iy[:, k], :] * cy[:, k, None]
    return v


def letterbox_cubic(frames, params, h, w):
    """frames [B, ..., H, W], params rows (nw, nh, dx, dy, flip) -> float64 [B, ..., h, w]"""
    frames = np.asarray(frames)
    out = np.zeros(frames.shape[:-2] + (h, w), dtype=np.float64)
    for b, (nw, nh, dx, dy, flip) in enumerate(np.asarray(params).reshape(-1, 5).tolist()):
        out[b, ..., dy:dy + nh, dx:dx + nw] = resize_cubic(frames[b], nw, nh)
        if flip:
            out[b] = out[b, ..., ::-1]
    return out
