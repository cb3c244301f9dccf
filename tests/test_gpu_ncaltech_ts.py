"""GPU tests of the N-Caltech101 front end's measure 'timesurface': ``ops.event_timesurface_atis`` against the fixture recorded from the
reference with measure='timesurface' (tests/golden/ncaltech_timesurface.npz; tests/ncaltech_ts_ref.py is pinned to it by
test_cpu_ncaltech_ts.py), its ties to the count entry (tau = 1e300: every weight is exactly 1), bit-reproducibility, ``ops.frames_letterbox``
against the restated cv2 rules, and the chain ``data.atis_to_frames`` -- eagerly and replayed from a captured graph -- with the measure taken
from an experiment's ``measure`` field, which the front end used to ignore.

Bounds.  A bin: |got - want| <= count * 2^-47 -- per event 2^-49 for the rounding of the weight to a multiple of 2^-48 plus 2 ulp of tanh
(<= 2^-52 below 1), doubled; a correct fp64 accumulation meets it too.  The letterboxed fp32 element: within one fp32 ulp of the letterboxed
fixture (a <= 1e-14 relative change of the input moves an fp32 rounding by at most one step), at least 99 % of the elements equal
(test_cpu_ncaltech_ts.py confirms both for the kernel's arithmetic restated in numpy)."""
import types

import numpy as np
import pytest
import torch

import ncaltech_ref
import ncaltech_ts_ref as ts_ref
from eas_snn_amd import _lib, data, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cases():
    return ts_ref.load_cases()


def on_device(dev, bufs, shift=0):
    """the recordings back to back, the byte image ``shift`` bytes behind an aligned address -> (records, offsets) on the device"""
    buf = np.concatenate(bufs)
    off = np.cumsum([0] + [len(b) // 5 for b in bufs]).astype(np.int64)
    store = torch.zeros(len(buf) + 8, dtype=torch.uint8, device=dev)
    assert store.data_ptr() % 16 == 0
    rec = store[shift:shift + len(buf)]
    rec.copy_(torch.from_numpy(buf))
    return rec, torch.from_numpy(off).to(dev)


def run_ts(dev, c, bufs=None, shift=0, tau=500e3):
    rec, off = on_device(dev, c['bufs'] if bufs is None else bufs, shift)
    frames, oob, flags = ops.event_timesurface_atis(rec, off, c['Tl'], c['Tm'], c['H'], c['W'], window=c['window'], tau=tau, return_oob=True,
                                                    return_flags=True)
    assert frames.dtype == torch.float64 and frames.shape == (off.numel() - 1, c['Tl'], c['Tm'], 2, c['H'], c['W'])
    return frames, oob, flags


def run_counts(dev, c, bufs=None):
    rec, off = on_device(dev, c['bufs'] if bufs is None else bufs)
    return ops.event_histogram_atis(rec, off, c['Tl'], c['Tm'], c['H'], c['W'], window=c['window'], return_oob=True, return_flags=True)


@pytest.mark.parametrize('name', ts_ref.CASES)
def test_frames_against_the_fixture(dev, cases, name):
    c = cases[name]
    frames, oob, flags = run_ts(dev, c)
    counts, c_oob, c_flags = run_counts(dev, c)
    got, want, n = frames.cpu().numpy(), c['frames'], counts.cpu().numpy()
    err = np.abs(got - want)
    print(f'{name}: worst bin error {err.max():.3e}, worst error per event {(err[n > 0] / n[n > 0]).max() * 2.0 ** 49:.3f} * 2^-49')
    assert (err <= n * 2.0 ** -47).all(), f'{int((err > n * 2.0 ** -47).sum())} bins beyond count * 2^-47, worst {err.max():.3e}'
    assert not got[n == 0].any() and (got[n > 0] > 0).all()
    # flags and out-of-sensor counts are the count entry's; no macro slice is longer than a bin's capacity
    assert torch.equal(oob, c_oob) and torch.equal(flags, c_flags) and not (flags & 4).any()
    assert max(len(b) // 5 for b in c['bufs']) <= _lib.lib().eas_event_timesurface_atis_capacity()
    # the same call twice
    again = run_ts(dev, c)
    assert all(torch.equal(a, b) for a, b in zip(again, (frames, oob, flags)))


@pytest.mark.parametrize('name', ['overflow_negwin_2x3', ts_ref.HOT])
def test_weights_of_one_give_the_count_path_bit_for_bit(dev, cases, name):
    """tau = 1e300: (t_target - t) / tau is below 2^-900, its tanh too, and 1 minus that rounds to 1: the instance of the histogram kernel
    and of the letterbox kernel on doubles against the pinned integer ones"""
    c = cases[name]
    frames, oob, flags = run_ts(dev, c, tau=1e300)
    counts, c_oob, c_flags = run_counts(dev, c)
    assert counts.sum() > 500 and torch.equal(frames, counts.double()) and torch.equal(oob, c_oob) and torch.equal(flags, c_flags)
    par = torch.from_numpy(ts_ref.case_params(len(c['bufs']))).to(dev)
    for interp in ('linear', 'cubic'):
        a, b = ops.frames_letterbox(frames, par, *ts_ref.CANVAS, interp=interp), ops.counts_letterbox(counts, par, *ts_ref.CANVAS, interp=interp)
        assert a.dtype == torch.float32 and a.shape == b.shape and torch.equal(a, b), interp


def test_hot_pixel_frames_do_not_depend_on_neighbours_or_alignment(dev, cases):
    """650 adds into one bin from six blocks' worth of records: alone, as recording 2 of a batch of 3, and with the byte buffer 1, 2 and 3
    bytes behind an aligned address"""
    c = cases[ts_ref.HOT]
    hot = c['bufs'][0]
    alone = run_ts(dev, c)
    assert int(run_counts(dev, c)[0].max()) >= 600
    others = cases['plain_1x4']['bufs']
    batch = [others[0], others[1], hot]
    for shift in (0, 1, 2, 3):
        one = run_ts(dev, c, shift=shift)
        three = run_ts(dev, c, bufs=batch, shift=shift)
        for a, b, w in zip(one, three, alone):
            assert torch.equal(a, w) and torch.equal(b[2:], w), f'base address + {shift} bytes'
    first = run_ts(dev, c, bufs=[hot, others[2], others[0]], shift=1)
    assert torch.equal(first[0][:1], alone[0])


def test_capacity_flag_fires_exactly_above_the_capacity(dev):
    """Flag bit 2 at its threshold, the one size at which the plan takes another path: a macro slice of capacity + 1 records sets it, one of
    exactly the capacity does not, and the longer recording cut into two macro slices does not either.  The events are spread over the
    sensor (no bin comes near its capacity: the flag is conservative); with tau = 1e300 the frames are the counts."""
    cap = int(_lib.lib().eas_event_timesurface_atis_capacity())
    H, W = 36, 48
    rng = np.random.default_rng(4)

    def recording(n):                    # n events at distinct times: the macro slice (Tl = 1) holds all but the last one
        return data.encode_atis(3 * np.arange(n), rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n))

    bufs = [recording(cap + 2), recording(cap + 1)]
    for Tl, want in ((1, [4, 0]), (2, [0, 0])):
        c = dict(bufs=bufs, window=None, Tl=Tl, Tm=4, H=H, W=W)
        frames, oob, flags = run_ts(dev, c, tau=1e300)
        counts, c_oob, c_flags = run_counts(dev, c)
        assert flags.tolist() == want and c_flags.tolist() == [0, 0] and torch.equal(oob, c_oob)
        assert torch.equal(frames, counts.double()) and int(counts[0].sum()) > cap - 4 * Tl


@pytest.mark.parametrize('interp', ['cubic', 'linear'])
def test_letterbox_of_float64_frames_equals_the_restated_rule(dev, cases, interp):
    """the kernel and the restatement do the same float64 operations in the same order: equal bit for bit"""
    for name in ('overflow_negwin_2x3', 'plain_1x4', ts_ref.HOT):
        want_frames = cases[name]['frames']
        par = ts_ref.case_params(len(want_frames))
        got = ops.frames_letterbox(torch.from_numpy(want_frames).to(dev), torch.from_numpy(par).to(dev), *ts_ref.CANVAS, interp=interp)
        want = ts_ref.letterbox(want_frames, par, *ts_ref.CANVAS, interp).astype(np.float32)
        assert got.shape == want.shape and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), want), f'{name}: {int((got.cpu().numpy() != want).sum())} elements differ'
        assert not np.array_equal(want, np.round(want)) and (interp == 'linear' or (want < 0).any())


def exp_like(c, measure):
    """the fields ``data.atis_to_frames`` reads of an experiment (yolox/exp/event_yolox_base.py); ``window`` is in ms there"""
    assert c['window'] is None or (c['window'][1] == 0 and c['window'][0] % 1000 == 0)
    window = None if c['window'] is None else c['window'][0] // 1000
    return types.SimpleNamespace(Tl=c['Tl'], Tm=c['Tm'], img_size=(c['H'], c['W']), input_size=ts_ref.CANVAS, window=window, measure=measure)


def assert_within_one_ulp(got, want, what):
    tiny = float(np.finfo(np.float32).tiny)
    got, want = got.astype(np.float64), want.astype(np.float64)
    diff = np.abs(got - want)
    equal = float((got == want).mean())
    print(f'{what}: {equal:.5f} of the elements equal, worst difference {float((diff / np.maximum(np.abs(want), tiny)).max()) * 2.0 ** 23:.3f} ulp')
    assert (diff <= 2.0 ** -23 * np.maximum(np.abs(want), tiny)).all(), what
    assert equal >= 0.99, what


@pytest.mark.parametrize('name', ts_ref.CASES)
def test_atis_to_frames_takes_the_measure_from_the_experiment(dev, cases, name):
    """``measure timesurface`` used to train on count frames without a word: the experiment's field decides now.  Count frames miss the
    fixture by >= 1e-6 per event (its weights are 0.86 .. 0.999998), far outside one fp32 ulp."""
    c = cases[name]
    if c['window'] is not None and (c['window'][1] != 0 or c['window'][0] >= 0):
        dims = (c['Tl'], c['Tm'], (c['H'], c['W']), ts_ref.CANVAS, c['window'])       # a window an experiment cannot state: the tuple form
        run = lambda rec, off, par, interp: data.atis_to_frames(rec, off, dims, par, interp=interp, measure='timesurface')
    else:
        exp = exp_like(c, 'timesurface')
        run = lambda rec, off, par, interp: data.atis_to_frames(rec, off, exp, par, interp=interp)
    rec, off = on_device(dev, c['bufs'])
    par = ts_ref.case_params(len(c['bufs']))
    for interp in ('cubic', 'linear'):
        want = ts_ref.letterbox(c['frames'], par, *ts_ref.CANVAS, interp).astype(np.float32)
        got = run(rec, off, par, interp)
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert_within_one_ulp(got.cpu().numpy(), want, f'{name} {interp}')


def test_count_measure_is_what_it_was(dev, cases):
    """measure 'count' -- stated, read from an experiment, or left out -- runs the count entry and the integer letterbox as before"""
    c = cases['overflow_negwin_2x3']
    rec, off = on_device(dev, c['bufs'])
    par = torch.from_numpy(ts_ref.case_params(len(c['bufs']))).to(dev)
    counts = ops.event_histogram_atis(rec, off, c['Tl'], c['Tm'], c['H'], c['W'], window=c['window'])
    want = ops.counts_letterbox(counts, par, *ts_ref.CANVAS, interp='cubic')
    dims = (c['Tl'], c['Tm'], (c['H'], c['W']), ts_ref.CANVAS, c['window'])
    assert torch.equal(data.atis_to_frames(rec, off, dims, par), want)
    assert torch.equal(data.atis_to_frames(rec, off, dims, par, measure='count'), want)
    assert torch.equal(data.atis_to_frames(rec, off, exp_like(c, 'count'), par), want)
    no_field = exp_like(c, 'count')
    del no_field.measure
    assert torch.equal(data.atis_to_frames(rec, off, no_field, par), want)
    assert not torch.equal(data.atis_to_frames(rec, off, exp_like(c, 'timesurface'), par), want)


def test_atis_to_frames_from_a_graph(dev, cases):
    c = cases[ts_ref.HOT]
    bufs = [cases['plain_1x4']['bufs'][0], cases['plain_1x4']['bufs'][2], c['bufs'][0]]
    rec, off = on_device(dev, bufs, shift=3)
    par = torch.from_numpy(ts_ref.case_params(3)).to(dev)
    exp = exp_like(c, 'timesurface')
    eager = data.atis_to_frames(rec, off, exp, par)
    assert eager.shape == (3, c['Tl'], c['Tm'], 2, *ts_ref.CANVAS) and eager.abs().sum() > 100
    side = _lib.private_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        data.atis_to_frames(rec, off, exp, par)                             # allocator warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            res = data.atis_to_frames(rec, off, exp, par)                   # no host read inside: the capture would fail
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        res.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(res, eager)
