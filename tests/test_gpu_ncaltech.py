"""GPU tests of the N-Caltech101 front end: ``ops.event_histogram_atis`` against the fixture recorded from the reference
(tests/golden/ncaltech_atis.npz) and against the numpy checker (tests/ncaltech_ref.py, pinned to that fixture by test_cpu_ncaltech.py),
the cubic letterbox against the checker's restatement of OpenCV's INTER_CUBIC (parity against cv2 unpinned), and the chain
``data.atis_to_frames`` eagerly and replayed from a captured graph.  Everything is integer counting or contraction-free float64
arithmetic, so every comparison is exact."""
import numpy as np
import pytest
import torch

from conftest import load_golden, split_cases

import ncaltech_ref
from eas_snn_amd import _lib, data, ops
from eas_snn_amd._lib import ptr, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def golden():
    return split_cases(load_golden('ncaltech_atis'))


def run_atis(dev, bufs, window, Tl, Tm, H, W, shift=0):
    """the recordings ``bufs`` in one call, the byte image placed ``shift`` bytes behind an aligned address -> numpy counts, oob, flags"""
    buf = np.concatenate(bufs) if len(bufs) else np.zeros(0, np.uint8)
    off = np.cumsum([0] + [len(b) // 5 for b in bufs]).astype(np.int64)
    store = torch.zeros(len(buf) + 8, dtype=torch.uint8, device=dev)
    assert store.data_ptr() % 16 == 0
    rec = store[shift:shift + len(buf)]
    rec.copy_(torch.from_numpy(buf))
    counts, oob, flags = ops.event_histogram_atis(rec, torch.from_numpy(off).to(dev), Tl, Tm, H, W, window=window, return_oob=True,
                                                  return_flags=True)
    assert counts.shape == (len(bufs), Tl, Tm, 2, H, W) and counts.dtype == torch.int32
    return counts.cpu().numpy(), oob.cpu().numpy(), flags.cpu().numpy()


def check_against_checker(got, bufs, window, Tl, Tm, H, W):
    counts, oob, flags = got
    for b, buf in enumerate(bufs):
        want, want_oob, want_flags = ncaltech_ref.atis_frames(buf, window, Tl, Tm, H, W)
        assert np.array_equal(counts[b], want), f'recording {b}: {int((counts[b] != want).sum())} counts differ'
        assert int(oob[b]) == want_oob and int(flags[b]) == want_flags, (b, int(oob[b]), want_oob, int(flags[b]), want_flags)


def random_recording(rng, n, H, W, span, overflow_at=(), t_first=None, ties=1):
    t = np.sort(rng.integers(0, span, n)) + (8192 * len(overflow_at) if t_first is None else t_first)
    t[n - ties:] = t[-1]
    return data.encode_atis(t, rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n), overflow_before=overflow_at)


@pytest.mark.parametrize('name', ['plain_1x4', 'window0_2x3', 'negwin_1x8', 'negwin_hi_2x3', 'overflow_1x4', 'overflow_negwin_2x3',
                                  'overflow_1x8', 'short_span_w0', 'polarity_1x4', 'polarity_2x3'])
def test_golden_counts_equal_the_reference(dev, golden, name):
    case = golden[name]
    Tl, Tm, H, W = (int(case[k]) for k in ('Tl', 'Tm', 'H', 'W'))
    window = tuple(int(v) for v in case['window']) if int(case['has_window']) else None
    off = case['offsets']
    bufs = [case['bytes'][5 * off[b]:5 * off[b + 1]] for b in range(len(off) - 1)]
    got = run_atis(dev, bufs, window, Tl, Tm, H, W)
    assert np.array_equal(got[0], case['frames'])
    check_against_checker(got, bufs, window, Tl, Tm, H, W)


def ragged_recordings():
    H, W = 20, 24
    rng = np.random.default_rng(11)
    n = 20_000
    marks = [0, 255, 256, 1023, 1024, 4095, 4096, n - 1]                   # record indices of the overflow records
    before = [m - k for k, m in enumerate(marks)]                           # = the event index each one stands in front of
    big = random_recording(rng, n - len(marks), H, W, 250_000, overflow_at=before, ties=3)
    assert len(big) == 5 * n and np.flatnonzero(big.reshape(-1, 5)[:, 1] == 240).tolist() == marks
    only_overflow = data.encode_atis([], [], [], [], overflow_before=(0,) * 7)
    return [np.zeros(0, np.uint8), random_recording(rng, 1, H, W, 1000), only_overflow, random_recording(rng, 3, H, W, 5000),
            random_recording(rng, 1001, H, W, 90_000, overflow_at=(500,)), big]


def test_ragged_batch_at_four_alignments(dev):
    """0 records, 1 event, only overflow records, 3 events, 1001 events, and 20 000 records with overflow records on both sides of every
    chunk boundary a power-of-two chunk up to 4096 has (the kernels' chunk is 256 records of the buffer: the second order, big
    recording first, puts those record indices on its boundaries too)"""
    H, W, Tl, Tm = 20, 24, 1, 4
    bufs = ragged_recordings()
    first = run_atis(dev, bufs, None, Tl, Tm, H, W)
    check_against_checker(first, bufs, None, Tl, Tm, H, W)
    assert first[2].tolist() == [2, 2, 2, 0, 0, 0] and not first[0][:3].any()
    # the parent's histogram on the host-decoded macro slice (t0 <= t < t0 + mw): pinned to the reference before this front end existed
    ev = [ncaltech_ref.decode_atis(b) for b in bufs]
    cut = []
    for t, x, y, p in ev:
        m = (t >= t[0]) & (t < t[0] + (t[-1] - t[0]) // Tl) if len(t) else np.zeros(0, bool)
        cut.append((t[m], x[m], y[m], p[m]))
    cat = lambda i, dt: torch.from_numpy(np.concatenate([c[i] for c in cut]).astype(dt)).to(dev)
    off = torch.from_numpy(np.cumsum([0] + [len(c[0]) for c in cut]).astype(np.int64)).to(dev)
    hist = ops.event_histogram(cat(0, np.int32), cat(1, np.int16), cat(2, np.int16), cat(3, np.uint8), off, Tm, H, W)
    assert np.array_equal(hist.cpu().numpy(), first[0][:, 0])
    for shift in (1, 2, 3):
        got = run_atis(dev, bufs, None, Tl, Tm, H, W, shift=shift)
        for a, b in zip(got, first):
            assert np.array_equal(a, b), f'base address + {shift} bytes'
    order = [5, 0, 1, 2, 3, 4]
    swapped = run_atis(dev, [bufs[i] for i in order], None, Tl, Tm, H, W, shift=1)
    for a, b in zip(swapped, first):
        assert np.array_equal(a, b[order])
    windowed = run_atis(dev, bufs, (-60_000, -1000), Tl, 3, H, W, shift=2)
    check_against_checker(windowed, bufs, (-60_000, -1000), Tl, 3, H, W)


def test_flags_and_out_of_sensor_events(dev):
    H, W, Tl, Tm = 20, 24, 1, 4
    rng = np.random.default_rng(5)
    n = 600
    t = np.sort(rng.integers(20_000, 90_000, n))
    x, y, p = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)
    drop = t.copy()
    drop[300:] -= 9000                                                      # the raw time drops once
    assert (np.diff(drop) < 0).sum() == 1
    x_bad, y_bad = x.copy(), y.copy()
    y_bad[10:40:3], y_bad[100], y_bad[200], x_bad[50:60] = H, 239, 241, W
    bufs = [data.encode_atis(drop, x, y, p, overflow_before=(0, 450)), np.zeros(0, np.uint8), data.encode_atis(t, x_bad, y_bad, p),
            data.encode_atis(t, x, y, p, overflow_before=(100,))]
    counts, oob, flags = run_atis(dev, bufs, None, Tl, Tm, H, W)
    assert int(flags[0]) & 1                                                # only the flag: the frames of that recording are unspecified
    assert int(flags[1]) == 2 and not counts[1].any()
    check_against_checker((counts[2:], oob[2:], flags[2:]), bufs[2:], None, Tl, Tm, H, W)
    binned = ncaltech_ref.atis_frames(bufs[3], None, Tl, Tm, H, W)[0].sum()
    assert int(oob[2]) > 15 and int(oob[3]) == 0 and int(flags[2]) == 0 and counts[2].sum() + int(oob[2]) == binned
    # without the optional outputs
    rec = torch.from_numpy(np.concatenate(bufs)).to(dev)
    off = torch.from_numpy(np.cumsum([0] + [len(b) // 5 for b in bufs]).astype(np.int64)).to(dev)
    plain = ops.event_histogram_atis(rec, off, Tl, Tm, H, W)
    assert np.array_equal(plain.cpu().numpy()[1:], counts[1:])


def test_two_macro_slices_take_their_windows_from_their_own_members(dev):
    H, W, Tl, Tm = 20, 24, 2, 3
    rng = np.random.default_rng(8)
    bufs = [random_recording(rng, 3000, H, W, 120_000, overflow_at=(0, 700, 701, 2999), ties=4),
            random_recording(rng, 257, H, W, 30_000), random_recording(rng, 2, H, W, 10), random_recording(rng, 700, H, W, 200_000)]
    for window in (None, (-50_000, 0)):
        check_against_checker(run_atis(dev, bufs, window, Tl, Tm, H, W), bufs, window, Tl, Tm, H, W)
    # the slices differ in their first member's time and in their micro window
    t = ncaltech_ref.decode_atis(bufs[0])[0]
    mw = (t[-1] - t[0]) // 2
    s0, s1 = t[t < t[0] + mw], t[(t >= t[0] + mw) & (t < t[0] + 2 * mw)]
    assert s1[0] != t[0] + mw or (s0[-1] - s0[0]) // Tm != (s1[-1] - s1[0]) // Tm


def test_cubic_letterbox(dev):
    B, H, W, Hc, Wc = 3, 18, 24, 24, 32
    rng = np.random.default_rng(2)
    counts = rng.integers(0, 12, (B, 4, 2, H, W)).astype(np.int32)         # F = 8 frames per sample
    counts[rng.random(counts.shape) < 0.6] = 0
    params = np.array([(32, 24, 0, 0, 0), (13, 9, 7, 5, 1), (24, 18, 0, 0, 0)], np.int32)
    c_dev, p_dev = torch.from_numpy(counts).to(dev), torch.from_numpy(params).to(dev)
    got = ops.counts_letterbox(c_dev, p_dev, Hc, Wc, interp='cubic')
    want = ncaltech_ref.letterbox_cubic(counts, params, Hc, Wc).astype(np.float32)
    assert got.shape == (B, 4, 2, Hc, Wc) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want), f'{int((got.cpu().numpy() != want).sum())} elements differ'
    assert (want[0] < 0).any() and not np.array_equal(want[0], np.round(want[0]))        # a cubic kernel overshoots
    assert torch.equal(got[2], ops.counts_to_canvas(c_dev[2], Hc, Wc))                   # the identity size is a copy
    linear = ops.counts_letterbox(c_dev, p_dev, Hc, Wc)
    assert torch.equal(linear, ops.counts_letterbox(c_dev, p_dev, Hc, Wc, interp='linear')) and not torch.equal(linear[0], got[0])
    ex = torch.full_like(linear, 7.0)
    _lib.check(_lib.lib().eas_counts_letterbox_ex(ptr(c_dev), ptr(p_dev), 0, B, 8, H, W, Hc, Wc, ptr(ex), stream()), 'eas_counts_letterbox_ex')
    assert torch.equal(ex, linear)
    assert _lib.lib().eas_counts_letterbox_ex(ptr(c_dev), ptr(p_dev), 2, B, 8, H, W, Hc, Wc, ptr(ex), stream()) != 0


def test_atis_to_frames_eager_and_from_a_graph(dev):
    sensor, canvas, Tl, Tm = (36, 48), (48, 64), 1, 4
    buf, off = data.synth_atis_batch(3, 5000, *sensor)
    par = np.array([data.letterbox_params(*sensor, *canvas), (40, 30, 11, 9, 1), data.letterbox_params(*sensor, *canvas)], np.int32)
    want = np.stack([ncaltech_ref.atis_frames(buf[5 * off[b]:5 * off[b + 1]], None, Tl, Tm, *sensor)[0] for b in range(3)])
    assert want.sum() > 14_000
    want = ncaltech_ref.letterbox_cubic(want, par, *canvas).astype(np.float32)
    rec, off_dev, par_dev = torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(par).to(dev)
    dims = (Tl, Tm, sensor, canvas)
    eager = data.atis_to_frames(rec, off_dev, dims, par)
    assert eager.shape == (3, Tl, Tm, 2, *canvas) and np.array_equal(eager.cpu().numpy(), want)
    side = _lib.private_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        data.atis_to_frames(rec, off_dev, dims, par_dev)                    # allocator warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            res = data.atis_to_frames(rec, off_dev, dims, par_dev)          # no host read inside: the capture would fail
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        res.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(res, eager)
