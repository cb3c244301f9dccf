"""Plain numpy checker of the 1 Mpx front end (eas_stacked_hist_frames): the index, ``lo`` and ``R`` rules of include/eas_hip.h written
out sample by sample around the oracle's own ``stacked_hist_event_sum`` (pinned to the reference's generate_slices by
tests/golden/stacked_hist.npz) and ``letterbox_frames`` (the image side of get_random_data), which are imported, not copied.
tests/test_cpu_gen4.py pins ``frames`` with identity params to every case of that fixture."""
import numpy as np

from oracle import events_ref


def slices_of(store, first, lo, Tm):
    """-> (the representations that exist among first .. first + Tm - 1 -- they are the LAST ones of the sample --, flag): indices below
    ``max(lo, 0)`` are the zero slices in front (rvt_gen4.py:119-124), indices >= R are never read: zero and flagged"""
    R = store.shape[0]
    first, lo = int(first), max(int(lo), 0)
    idx = [first + j for j in range(Tm)]
    flag = int(any(i >= lo and i >= R for i in idx))
    return idx, lo, R, flag


def sample_counts(store, first, lo, Tm, nbins):
    """float64 [Tm, 2, H, W] bin sums of one sample + flag"""
    H, W = store.shape[-2:]
    idx, lo, R, flag = slices_of(store, first, lo, Tm)
    out = np.zeros((Tm, 2, H, W))
    have = [j for j, i in enumerate(idx) if lo <= i < R]
    # runs of existing slices are contiguous; each run goes through the oracle as the reference would read it (its own front padding
    # is the rule for indices below lo; slices behind the end stay zero)
    if have:
        a, b = have[0], have[-1] + 1
        assert have == list(range(a, b))
        got = events_ref.stacked_hist_event_sum(store[idx[a]:idx[b - 1] + 1], b, H, W)[0]        # [b, 2, H, W], zero slices in front
        assert store.shape[1] == 2 * nbins
        out[:b] = got
    return out, flag


def paste(frames, params, h, w):
    """``events_ref.letterbox_frames`` for any (nw, nh, dx, dy, flip): an empty rectangle (nw <= 0 or nh <= 0) is a zero canvas, a
    rectangle that leaves the canvas is clipped -- the resized image is pasted on a canvas large enough to hold it, the part on
    [0, h) x [0, w) is kept, and the flip mirrors that"""
    nw, nh, dx, dy, flip = (int(v) for v in params)
    nf, nc = frames.shape[:2]
    if nw <= 0 or nh <= 0:
        return np.zeros((nf, nc, h, w))
    ox, oy = max(0, -dx), max(0, -dy)                    # shift so that the paste position is non-negative
    bh, bw = max(h + oy, dy + oy + nh), max(w + ox, dx + ox + nw)
    big = events_ref.letterbox_frames(frames, (nw, nh, dx + ox, dy + oy, 0), bh, bw)
    out = np.ascontiguousarray(big[:, :, oy:oy + h, ox:ox + w])
    return np.ascontiguousarray(out[..., ::-1]) if flip else out


def frames(store, first, Tm, Hc, Wc, nbins=10, lo=None, params=None):
    """-> (float32 [B, 1, Tm, 2, Hc, Wc], flags uint32 [B]) as eas_stacked_hist_frames defines them"""
    store = np.asarray(store)
    B = len(first)
    H, W = store.shape[-2:]
    out = np.zeros((B, 1, Tm, 2, Hc, Wc), dtype=np.float32)
    flags = np.zeros(B, dtype=np.uint32)
    for b in range(B):
        counts, flags[b] = sample_counts(store, first[b], 0 if lo is None else lo[b], Tm, nbins)
        par = (W, H, 0, 0, 0) if params is None else params[b]
        out[b, 0] = paste(counts, par, Hc, Wc).astype(np.float32)
    return out, flags
