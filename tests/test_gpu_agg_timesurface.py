"""GPU tests of ``aggregation timesurface`` on the device front ends: ``ops.event_latest_surface_atis`` against the fixture recorded from the
reference's agrregate(aggregation='timesurface') (tests/golden/ncaltech_agg_timesurface.npz; tests/agg_ts_ref.py is pinned to it, bit for
bit, by test_cpu_agg_timesurface.py), ``ops.event_latest_surface_dat_ranges`` against the reference outputs of
tests/golden/events_time_surface.npz re-encoded to .dat records, the chains of ``eas_snn_amd.data`` that consult the option -- eagerly and
replayed from a captured graph -- and the synthetic loaders, which used to ignore it.

Bounds.  A surface against the fixture / oracle: rtol = 1e-13, atol = 0, the bar of test_time_surface_golden_and_batch -- the division by
tau rounds the exponent x by <= 2^-53 |x| (|x| <= 100 asserted by the fixture's generator; <= 120 for the Gen1 fixture), exp adds <= 2 ulp:
about 1.2e-14.  The integer part is exact: rint(log(got) * tau) == rint(log(want) * tau) elementwise.  A letterboxed fp32 element against
the letterbox of the fixture in float64: |got - want| <= 2^-23 |want| + 1e-12 -- one fp32 rounding step plus the 1e-13 input error times the
sum of the absolute 2-D cubic tap weights (<= 1.9) at values <= 1, rounded up."""
import types

import numpy as np
import pytest
import torch

import agg_ts_ref as ref
import ncaltech_ref
import ncaltech_ts_ref as ts_ref
from conftest import load_golden, split_cases
from eas_snn_amd import _lib, data, ops
from oracle import events_ref

pytestmark = pytest.mark.gpu

TAU = 10e3
GEN1_HW, GEN1_CANVAS = (24, 32), (32, 40)
# (nw, nh, dx, dy, flip) on the 32 x 40 canvas for the 24 x 32 sensor: scaled up, shrunk and mirrored at an offset, the identity size at an offset
GEN1_PARAMS = [(40, 30, 0, 1, 0), (24, 18, 7, 5, 1), (32, 24, 3, 2, 0)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cases():
    return ref.load_cases()


@pytest.fixture(scope='module')
def gen1():
    """the cases of events_time_surface.npz with their events re-encoded to .dat records (header stripped): name -> dict(..., rec uint8)"""
    out = {}
    for name, c in split_cases(load_golden('events_time_surface')).items():
        image = events_ref.encode_dat_file(c['t'], c['x'], c['y'], c['p'], int(c['H']), int(c['W']))
        start, ev_type, ev_size = events_ref.parse_dat_header(image)
        assert ev_size == 8 and (len(image) - start) == 8 * len(c['t'])
        out[name] = dict(c, rec=np.frombuffer(image[start:], dtype=np.uint8).copy())
    return out


def assert_surface(got, want, tau, what):
    """rtol 1e-13 and the exact integer part; prints the worst relative error"""
    assert got.shape == want.shape and got.dtype == np.float64
    rel = np.abs(got - want) / want
    print(f'{what}: worst relative error {rel.max():.3e}')
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0, err_msg=what)
    assert np.array_equal(np.rint(np.log(got) * tau), np.rint(np.log(want) * tau)), what


def assert_letterboxed(got, want, what):
    got, want = got.astype(np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    diff, bound = np.abs(got - want), 2.0 ** -23 * np.abs(want) + 1e-12
    print(f'{what}: worst difference {diff.max():.3e}, worst share of the bound {(diff / bound).max():.3f}')
    assert (diff <= bound).all(), what


def on_device(dev, bufs, shift=0):
    """the recordings back to back, the byte image ``shift`` bytes behind an aligned address -> (records, offsets) on the device"""
    buf = np.concatenate(bufs)
    off = np.cumsum([0] + [len(b) // 5 for b in bufs]).astype(np.int64)
    store = torch.zeros(len(buf) + 8, dtype=torch.uint8, device=dev)
    assert store.data_ptr() % 16 == 0
    rec = store[shift:shift + len(buf)]
    rec.copy_(torch.from_numpy(buf))
    return rec, torch.from_numpy(off).to(dev)


def run_latest(dev, c, bufs=None, shift=0, tau=TAU):
    rec, off = on_device(dev, c['bufs'] if bufs is None else bufs, shift)
    frames, oob, flags = ops.event_latest_surface_atis(rec, off, c['Tl'], c['Tm'], c['H'], c['W'], window=c['window'], tau=tau, return_oob=True,
                                                       return_flags=True)
    assert frames.dtype == torch.float64 and frames.shape == (off.numel() - 1, c['Tl'], c['Tm'], 2, c['H'], c['W'])
    return frames, oob, flags


def replayed(fn):
    """``fn()`` captured into a graph on a private stream and replayed twice -> the result tensor of the last replay"""
    side = _lib.private_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                                                # allocator warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            res = fn()                                                      # no host read inside: the capture would fail
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        res.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
    return res


# ------------------------------------------------------------------------------------------------ ATIS records
@pytest.mark.parametrize('name', ref.CASES)
def test_atis_frames_against_the_fixture(dev, cases, name):
    c = cases[name]
    frames, oob, flags = run_latest(dev, c)
    rec, off = on_device(dev, c['bufs'])
    _, c_oob, c_flags = ops.event_histogram_atis(rec, off, c['Tl'], c['Tm'], c['H'], c['W'], window=c['window'], return_oob=True, return_flags=True)
    got, raises = frames.cpu().numpy(), c['raises'].astype(bool)
    # bit 3 exactly where the reference raised, zero frames there; bits 0 and 1 and the out-of-sensor counts are the count entry's
    assert ((flags.cpu().numpy() & 8) != 0).tolist() == raises.tolist() and not got[raises].any()
    assert torch.equal(flags & ~8, c_flags) and not oob.any() and torch.equal(oob, c_oob)
    assert_surface(got[~raises], c['frames'][~raises], TAU, name)
    assert (got[~raises] > 0).all() and (got[~raises] < 1).all()
    again = run_latest(dev, c)
    assert all(torch.equal(a, b) for a, b in zip(again, (frames, oob, flags)))


def test_atis_frames_do_not_depend_on_neighbours_or_alignment(dev, cases):
    """a recording with overflow records alone, as recording 2 of a batch of three, first of three, and with the byte image 1 .. 4 bytes
    behind an aligned address: the same bits"""
    c = cases[ref.HOT]
    hot, others = c['bufs'][0], cases['plain_1x4']['bufs']
    alone = run_latest(dev, c)
    for shift in (0, 1, 2, 3, 4):
        one = run_latest(dev, c, shift=shift)
        three = run_latest(dev, c, bufs=[others[0], others[1], hot], shift=shift)
        for a, b, w in zip(one, three, alone):
            assert torch.equal(a, w) and torch.equal(b[2:], w), f'base address + {shift} bytes'
    first = run_latest(dev, c, bufs=[hot, others[2], others[0]], shift=1)
    assert torch.equal(first[0][:1], alone[0])
    # the window-0 recording next to others: its flag and its zeros stay its own
    w0 = cases['short_span_w0']
    mixed = run_latest(dev, w0, bufs=[others[2], w0['bufs'][0], w0['bufs'][1]])
    assert (mixed[2] & 8).tolist() == [0, 8, 0] and not mixed[0][1].any() and (mixed[0][[0, 2]] > 0).all()


def test_atis_event_outside_the_sensor_is_dropped_and_counted(dev, cases):
    c = cases['plain_1x4']
    buf = c['bufs'][0].copy()
    t, x, y, p = ncaltech_ref.decode_atis(buf)                  # no overflow records: event i is record i
    i = len(t) // 2
    pixel = (slice(None), slice(None), slice(None), int(p[i] != 0), int(y[i]), int(x[i]))
    moved = buf.copy()
    moved[5 * i] = 200                                          # x = 200 on a 48-wide sensor
    want, want_oob, want_flags = ref.atis_latest_surface(moved, c['window'], c['Tl'], c['Tm'], c['H'], c['W'])
    assert want_oob == 1 and want_flags == 0
    base = run_latest(dev, c, bufs=[buf])[0].cpu().numpy()
    frames, oob, flags = run_latest(dev, c, bufs=[moved])
    got = frames.cpu().numpy()
    assert oob.tolist() == [1] and flags.tolist() == [0]
    assert_surface(got[0], want, TAU, 'one event moved outside')
    keep = np.ones(got.shape, dtype=bool)
    keep[pixel] = False
    assert np.array_equal(got[keep], base[keep]) and not np.array_equal(got[pixel], base[pixel])


def test_atis_pixel_hit_in_micro_slice_0_only_decays_as_the_formula_says(dev, cases):
    c = cases['plain_1x4']
    buf = c['bufs'][2]                                          # 90 events, Tl = 1, no window
    Tm, H, W = c['Tm'], c['H'], c['W']
    t, x, y, p = ncaltech_ref.decode_atis(buf)
    f = int(t[0])
    members = t[t < f + (int(t[-1]) - f)]                       # the macro slice: [t0, t0 + (tL - t0))
    w = (int(members[-1]) - f) // Tm
    counts = ncaltech_ref.atis_frames(buf, None, 1, Tm, H, W)[0][0]
    only0 = np.argwhere((counts[0] > 0) & (counts[1:].sum(axis=0) == 0))
    assert w > 0 and len(only0) > 3
    ticks = ref.exponent_ticks(run_latest(dev, c, bufs=[buf])[0].cpu().numpy()[0, 0])
    for ch, yy, xx in only0.tolist():
        latest = int(t[(x == xx) & (y == yy) & ((p != 0) == ch) & (t < f + w)].max())
        assert ticks[:, ch, yy, xx].tolist() == [latest - ((q + 1) * w + f) for q in range(Tm)]
    untouched = np.argwhere(counts.sum(axis=0) == 0)[0]
    assert ticks[(slice(None),) + tuple(untouched)].tolist() == [-((q + 1) * w + f) for q in range(Tm)]


# ------------------------------------------------------------------------------------------------ Gen1 .dat record ranges
def decoded_on_device(dev, streams):
    """[(t, x, y, p)] -> the concatenated arrays and offsets ``ops.event_time_surface`` takes"""
    cat = [torch.from_numpy(np.concatenate([s[k] for s in streams])).to(dev) for k in range(4)]
    off = torch.from_numpy(np.cumsum([0] + [len(s[0]) for s in streams]).astype(np.int64)).to(dev)
    return cat + [off]


def test_dat_ranges_every_case_of_the_fixture(dev, gen1):
    for name, c in gen1.items():
        ns, H, W, tau, n = int(c['ns']), int(c['H']), int(c['W']), float(c['tau']), len(c['t'])
        rec = torch.from_numpy(c['rec']).to(dev)
        ranges = torch.tensor([[0, n]], dtype=torch.int64, device=dev)
        out, oob = ops.event_latest_surface_dat_ranges(rec, ranges, ns, H, W, tau=tau, return_oob=True)
        assert out.dtype == torch.float64 and out.shape == (1, ns, 2, H, W) and oob.tolist() == [0]
        assert_surface(out[0].cpu().numpy(), c['out'], tau, name)
        same = ops.event_time_surface(*decoded_on_device(dev, [(c['t'], c['x'], c['y'], c['p'])]), ns, H, W, tau=tau)
        assert torch.equal(out, same), name
        assert torch.equal(ops.event_latest_surface_dat_ranges(rec, ranges, ns, H, W, tau=tau), out)


def test_dat_ranges_batch_empty_and_overlapping_ranges(dev, gen1):
    """three cases in one buffer, an empty range between them, and two overlapping ranges of the first case: [0, n) and [n / 3, n)"""
    (H, W), ns, tau = GEN1_HW, 4, 50e3
    parts = [gen1[k] for k in ('ts_small_n4', 'ts_small_n8', 'ts_small_n3_signed')]
    rec = torch.from_numpy(np.concatenate([q['rec'] for q in parts])).to(dev)
    start = np.cumsum([0] + [len(q['t']) for q in parts])
    n = len(parts[0]['t'])
    ranges = [(start[0], start[1]), (start[1], start[2]), (start[2], start[2]), (start[2], start[3]), (0, n), (n // 3, n)]
    streams = [tuple(q[k] for k in 'txyp') for q in parts]
    streams = [streams[0], streams[1], tuple(v[:0] for v in streams[0]), streams[2], streams[0], tuple(v[n // 3:] for v in streams[0])]
    out, oob = ops.event_latest_surface_dat_ranges(rec, torch.tensor(ranges, dtype=torch.int64, device=dev), ns, H, W, tau=tau, return_oob=True)
    got = out.cpu().numpy()
    assert oob.tolist() == [0] and not got[2].any() and np.array_equal(got[0], got[4])
    for b, s in enumerate(streams):
        if len(s[0]):
            assert_surface(got[b], events_ref.time_surface(*s, ns, H, W, tau), tau, f'range {b}')
    assert_surface(got[0], parts[0]['out'], tau, 'range 0 against the fixture')
    assert torch.equal(out, ops.event_time_surface(*decoded_on_device(dev, streams), ns, H, W, tau=tau))
    # a smaller sensor: the events outside it that would have been binned are dropped and counted
    h, w = H - 4, W - 5
    small, oob = ops.event_latest_surface_dat_ranges(rec, torch.tensor(ranges, dtype=torch.int64, device=dev), ns, h, w, tau=tau, return_oob=True)
    outside = 0
    for t, x, y, p in streams:
        if len(t):
            win = (int(t[-1]) - int(t[0])) // ns
            outside += int((((t.astype(np.int64) - int(t[0])) // win < ns) & ((x >= w) | (y >= h))).sum())
    assert outside > 100 and oob.tolist() == [outside]
    assert torch.equal(small, ops.event_time_surface(*decoded_on_device(dev, streams), ns, h, w, tau=tau))


# ------------------------------------------------------------------------------------------------ chains
def exp_like(c, **fields):
    """the fields ``data.atis_to_frames`` reads of an experiment (yolox/exp/event_yolox_base.py); ``window`` is in ms there"""
    assert c['window'] is None or (c['window'][1] == 0 and c['window'][0] % 1000 == 0)
    window = None if c['window'] is None else c['window'][0] // 1000
    return types.SimpleNamespace(Tl=c['Tl'], Tm=c['Tm'], img_size=(c['H'], c['W']), input_size=ts_ref.CANVAS, window=window, **fields)


@pytest.mark.parametrize('name', ref.CASES)
def test_atis_to_frames_takes_the_aggregation_from_the_experiment(dev, cases, name):
    """``aggregation timesurface`` used to train on count frames without a word: the experiment's field decides now.  The jitter-style
    params of ts_ref.PARAMS: scaled up, shrunk and mirrored, the identity size."""
    c = cases[name]
    if c['window'] is not None and (c['window'][1] != 0 or c['window'][0] >= 0):
        dims = (c['Tl'], c['Tm'], (c['H'], c['W']), ts_ref.CANVAS, c['window'])       # a window an experiment cannot state: the tuple form
        run = lambda rec, off, par, interp: data.atis_to_frames(rec, off, dims, par, interp=interp, aggregation='timesurface')
    else:
        exp = exp_like(c, aggregation='timesurface', measure='timesurface')            # the measure is not consulted
        run = lambda rec, off, par, interp: data.atis_to_frames(rec, off, exp, par, interp=interp)
    rec, off = on_device(dev, c['bufs'])
    par = ts_ref.case_params(len(c['bufs']))
    for interp in ('cubic', 'linear'):
        got = run(rec, off, par, interp)
        assert got.dtype == torch.float32 and got.shape == (len(c['bufs']), c['Tl'], c['Tm'], 2, *ts_ref.CANVAS)
        assert_letterboxed(got.cpu().numpy(), ts_ref.letterbox(c['frames'], par, *ts_ref.CANVAS, interp), f'{name} {interp}')


def test_atis_chain_from_a_graph_and_micro_sum_as_before(dev, cases):
    c = cases[ref.HOT]
    bufs = [cases['plain_1x4']['bufs'][0], cases['plain_1x4']['bufs'][2], c['bufs'][0]]
    rec, off = on_device(dev, bufs, shift=3)
    par = torch.from_numpy(ts_ref.case_params(3)).to(dev)
    for interp in ('cubic', 'linear'):
        exp = exp_like(c, aggregation='timesurface')
        eager = data.atis_to_frames(rec, off, exp, par, interp=interp)
        assert eager.shape == (3, c['Tl'], c['Tm'], 2, *ts_ref.CANVAS) and eager.abs().sum() > 100
        assert torch.equal(replayed(lambda: data.atis_to_frames(rec, off, exp, par, interp=interp)), eager), interp
        # 'micro_sum' -- stated, read from the experiment, or no field at all -- is the count entry and the integer letterbox, bit for bit
        counts = ops.event_histogram_atis(rec, off, c['Tl'], c['Tm'], c['H'], c['W'], window=c['window'])
        want = ops.counts_letterbox(counts, par, *ts_ref.CANVAS, interp=interp)
        assert torch.equal(data.atis_to_frames(rec, off, exp_like(c, aggregation='micro_sum'), par, interp=interp), want)
        assert torch.equal(data.atis_to_frames(rec, off, exp_like(c), par, interp=interp), want)
        assert torch.equal(data.atis_to_frames(rec, off, exp, par, interp=interp, aggregation='micro_sum'), want)
        assert not torch.equal(eager, want)


def test_dat_ranges_to_frames(dev, gen1):
    (H, W), (Hc, Wc), ns, tau = GEN1_HW, GEN1_CANVAS, 4, 50e3
    c = gen1['ts_small_n4']
    n = len(c['t'])
    rec = torch.from_numpy(c['rec']).to(dev)
    ranges = torch.tensor([(0, n), (n // 3, n), (0, n)], dtype=torch.int64, device=dev)
    par = np.array(GEN1_PARAMS, np.int32)
    sub = events_ref.time_surface(*(c[k][n // 3:] for k in 'txyp'), ns, H, W, tau)
    want = ts_ref.letterbox(np.stack([c['out'], sub, c['out']]), par, Hc, Wc, 'linear')[:, None]
    run = lambda: data.dat_ranges_to_frames(rec, ranges, ns, (H, W), (Hc, Wc), par_dev, aggregation='timesurface', tau=tau)
    par_dev = torch.from_numpy(par).to(dev)
    eager = run()
    assert eager.dtype == torch.float32 and eager.shape == (3, 1, ns, 2, Hc, Wc)
    assert_letterboxed(eager.cpu().numpy(), want, 'dat_ranges_to_frames')
    assert torch.equal(data.dat_ranges_to_frames(rec, ranges, ns, (H, W), (Hc, Wc), par, aggregation='timesurface', tau=tau), eager)
    assert torch.equal(replayed(run), eager)
    counts = ops.counts_letterbox(ops.event_histogram_dat_ranges(rec, ranges, ns, H, W), par_dev, Hc, Wc).unsqueeze(1)
    assert torch.equal(data.dat_ranges_to_frames(rec, ranges, ns, (H, W), (Hc, Wc), par_dev), counts)
    assert torch.equal(data.dat_ranges_to_frames(rec, ranges, ns, (H, W), (Hc, Wc), par_dev, aggregation='micro_sum'), counts)
    assert torch.equal(replayed(lambda: data.dat_ranges_to_frames(rec, ranges, ns, (H, W), (Hc, Wc), par_dev)), counts)
    # the chain from decoded events with the same option
    ev = dict(zip(('t', 'x', 'y', 'p', 'offsets'), decoded_on_device(dev, [tuple(c[k] for k in 'txyp'), tuple(c[k][n // 3:] for k in 'txyp'),
                                                                           tuple(c[k] for k in 'txyp')])))
    assert torch.equal(data.events_to_frames_augmented(ev, ns, (H, W), (Hc, Wc), par_dev, aggregation='timesurface', tau=tau), eager)
    assert torch.equal(data.events_to_frames_augmented(ev, ns, (H, W), (Hc, Wc), par_dev), counts)


# ------------------------------------------------------------------------------------------------ loaders
def test_synthetic_loaders_follow_the_experiment(dev):
    (H, W), (Hc, Wc), Tm, n_events, batch = (48, 60), (64, 64), 4, 2000, 2
    exp = types.SimpleNamespace(Tm=Tm, input_size=(Hc, Wc), test_size=(Hc, Wc), num_classes=2)
    ev_np = data.synth_event_batch(batch, n_events, H, W, seed=0)
    ev = data.events_to_device(ev_np, dev)
    counts = data.events_to_frames(ev, Tm, (H, W), (Hc, Wc))                       # the call the loader made before it read the option
    assert torch.equal(counts, ops.event_frames(ev['t'], ev['x'], ev['y'], ev['p'], ev['offsets'], Tm, H, W, Hc, Wc).unsqueeze(1))
    for aggregation in (None, 'micro_sum'):
        if aggregation:
            exp.aggregation = aggregation
        frames, targets = next(iter(data.SyntheticEventLoader(exp, batch, iters=1, n_events=n_events, sensor_hw=(H, W))))
        assert torch.equal(frames, counts) and targets.shape == (batch, 50, 5)
    exp.aggregation = 'timesurface'
    frames, _ = next(iter(data.SyntheticEventLoader(exp, batch, iters=1, n_events=n_events, sensor_hw=(H, W))))
    chain = data.events_to_frames(ev, Tm, (H, W), (Hc, Wc), aggregation='timesurface')
    assert frames.dtype == torch.float32 and frames.shape == counts.shape == (batch, 1, Tm, 2, Hc, Wc)
    assert torch.equal(frames, chain) and not torch.equal(frames, counts)
    assert torch.equal(replayed(lambda: data.events_to_frames(ev, Tm, (H, W), (Hc, Wc), aggregation='timesurface')), chain)
    # placed as the count frames are: scale 1, top left, zero padding
    off = ev_np['offsets']
    want = np.zeros((batch, 1, Tm, 2, Hc, Wc))
    for b in range(batch):
        want[b, 0, :, :, :H, :W] = events_ref.time_surface(*(ev_np[k][off[b]:off[b + 1]] for k in 'txyp'), Tm, H, W, 50e3)
    assert_letterboxed(frames.cpu().numpy(), want, 'SyntheticEventLoader timesurface')
    assert not frames[..., H:, :].any() and not frames[..., W:].any() and (frames[..., :H, :W] > 0).all()
    # the evaluation loader: sample i is the seeded stream 10 000 + i
    ids = [3, 5]
    parts = [data.synth_event_batch(1, n_events, H, W, seed=10_000 + i) for i in ids]
    cat = {k: np.concatenate([q[k] for q in parts]) for k in ('t', 'x', 'y', 'p')}
    cat['offsets'] = np.arange(len(ids) + 1, dtype=np.int64) * n_events
    ev2 = data.events_to_device(cat, dev)
    for aggregation in ('timesurface', 'micro_sum'):
        exp.aggregation = aggregation
        got = next(iter(data.SyntheticEvalLoader(exp, batch, ids, n_events=n_events, sensor_hw=(H, W))))[0]
        assert torch.equal(got, data.events_to_frames(ev2, Tm, (H, W), (Hc, Wc), aggregation=aggregation)), aggregation
    assert torch.equal(got, data.events_to_frames(ev2, Tm, (H, W), (Hc, Wc)))
