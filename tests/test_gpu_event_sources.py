"""What the event front ends' sources have in common, pinned across them: the three count sources (decoded arrays, .dat records with
offsets, .dat record ranges) give the same frames and the same out-of-sensor count, the latest-time surface of .dat ranges and of decoded
arrays drop the same events, the polarity byte of decoded arrays keeps its two readings (count: ``p != 0`` is channel 1; latest time:
``p > 1`` is dropped), a window of zero length gives zeros without touching the neighbouring sample, and the ATIS count and latest-time
entries report the same out-of-sensor counts and flag bits 0 and 1.  Everything is integer or compared between two device results, so
every comparison is exact.  A few thousand events on a 60 x 76 or 24 x 32 sensor per case."""
import numpy as np
import pytest
import torch

from eas_snn_amd import _lib, data, ops
from oracle import events_ref

pytestmark = pytest.mark.gpu

TM = 4
H, W = 60, 76
SIZES = (1001, 0, 3, 2500, 1)          # the ragged batch of test_event_histogram_from_dat_records


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


def dat_records(t, x, y, p, height, width):
    """the record area of a .dat image of the events, numpy uint8 [8 * n]"""
    image = events_ref.encode_dat_file(t, x, y, p, height, width)
    return np.frombuffer(image[events_ref.parse_dat_header(image)[0]:], dtype=np.uint8).copy()


def decoded(dev, t, x, y, p, offsets, shift=0):
    """the five arrays on the device, ``shift`` elements behind an aligned address (shift = 1: no vector loads)"""
    def put(a):
        return torch.from_numpy(np.concatenate([np.zeros(shift, dtype=a.dtype), a])).to(dev)[shift:]
    return put(t), put(x), put(y), put(p), torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(dev)


@pytest.fixture(scope='module')
def batch(dev):
    """the ragged batch, decoded and as one .dat image; ranges = the offset pairs + the overlapping range [n / 3, n) of sample 0"""
    streams = [events_ref.synth_events(n, H, W, seed=40 + i) for i, n in enumerate(SIZES)]
    t, x, y, p = (np.concatenate([s[j] for s in streams]) for j in range(4))
    offsets = np.cumsum([0] + list(SIZES)).astype(np.int64)
    pairs = np.stack([offsets[:-1], offsets[1:]], axis=1)
    ranges = np.concatenate([pairs, [[SIZES[0] // 3, SIZES[0]]]]).astype(np.int64)
    return dict(t=t, x=x, y=y, p=p, offsets=offsets, rec=torch.from_numpy(dat_records(t, x, y, p, H, W)).to(dev),
                pairs=torch.from_numpy(pairs).to(dev), ranges=torch.from_numpy(ranges).to(dev))


def outside_after_the_tail_rule(b, h, w):
    """numpy: events of the batch that the window keeps (win > 0, slice index < Tm) and that fall outside an h x w sensor"""
    n = 0
    for a, e in zip(b['offsets'][:-1], b['offsets'][1:]):
        if e <= a:
            continue
        t = b['t'][a:e].astype(np.int64)
        win = (t[-1] - t[0]) // TM
        if win == 0:
            continue
        keep = (t - t[0]) // win < TM
        n += int((keep & ((b['x'][a:e] >= w) | (b['y'][a:e] >= h))).sum())
    return n


def test_three_count_sources_give_the_same_frames(dev, batch):
    b = batch
    B = len(SIZES)
    want = ops.event_histogram(*decoded(dev, b['t'], b['x'], b['y'], b['p'], b['offsets']), TM, H, W)
    assert want.shape == (B, TM, 2, H, W) and int(want.sum()) > 0
    assert not want[1].any() and not want[4].any()                       # no events; one event: a window of zero length
    # the scatter form without its vector loads (arrays one element behind an aligned address)
    assert torch.equal(ops.event_histogram(*decoded(dev, b['t'], b['x'], b['y'], b['p'], b['offsets'], shift=1), TM, H, W), want)
    assert torch.equal(ops.event_histogram_dat(b['rec'], torch.from_numpy(b['offsets']).to(dev), TM, H, W), want)
    got = ops.event_histogram_dat_ranges(b['rec'], b['ranges'], TM, H, W)
    assert got.shape == (B + 1, TM, 2, H, W) and torch.equal(got[:B], want)
    # the overlapping range [n / 3, n) of sample 0 is the histogram of that slice alone, next to its neighbours or by itself
    a, e = SIZES[0] // 3, SIZES[0]
    alone = ops.event_histogram(*decoded(dev, b['t'][a:e], b['x'][a:e], b['y'][a:e], b['p'][a:e], [0, e - a]), TM, H, W)
    assert torch.equal(got[B], alone[0]) and torch.equal(ops.event_histogram_dat_ranges(b['rec'], b['ranges'][B:], TM, H, W), alone)
    # empty ranges (begin == end, end < begin) give zeros
    empty = torch.tensor([[7, 7], [9, 2]], dtype=torch.int64, device=dev)
    assert not ops.event_histogram_dat_ranges(b['rec'], empty, TM, H, W).any()
    # through the C ABI into an ``out`` filled with a sentinel: every element is written
    out = torch.full((B + 1, TM, 2, H, W), -7, dtype=torch.int32, device=dev)
    rc = _lib.lib().eas_event_histogram_dat_ranges(_lib.ptr(b['rec']), _lib.ptr(b['ranges']), B + 1, TM, H, W, _lib.ptr(out), None, _lib.stream())
    assert rc == 0 and torch.equal(out, got)


def test_every_source_counts_the_same_events_outside_the_sensor(dev, batch):
    b = batch
    h, w = H - 4, W - 5
    want = outside_after_the_tail_rule(b, h, w)
    assert want > 100
    offs = torch.from_numpy(b['offsets']).to(dev)
    c0, oob0 = ops.event_histogram(*decoded(dev, b['t'], b['x'], b['y'], b['p'], b['offsets']), TM, h, w, return_oob=True)
    c1, oob1 = ops.event_histogram_dat(b['rec'], offs, TM, h, w, return_oob=True)
    c2, oob2 = ops.event_histogram_dat_ranges(b['rec'], b['pairs'], TM, h, w, return_oob=True)
    _, oob3 = ops.event_latest_surface_dat_ranges(b['rec'], b['pairs'], TM, h, w, return_oob=True)
    assert [int(o) for o in (oob0, oob1, oob2, oob3)] == [want] * 4
    assert torch.equal(c1, c0) and torch.equal(c2, c0)
    assert int(c0.sum()) == outside_after_the_tail_rule(b, 0, 0) - want      # kept events = inside + outside


def test_polarity_byte_of_decoded_arrays(dev):
    """interior events with p in {2, 255}: the count takes them as channel 1 (p != 0), the latest-time surface drops them"""
    h, w, n = 24, 32, 2000
    t, x, y, p = events_ref.synth_events(n, h, w, seed=7)
    odd = np.zeros(n, dtype=bool)
    odd[5:n - 5:3] = True
    p = p.copy()
    p[odd] = np.where(np.arange(odd.sum()) % 2 == 0, 2, 255).astype(np.uint8)
    assert p[0] <= 1 and p[-1] <= 1 and (p == 2).any() and (p == 255).any()
    counts = ops.event_histogram(*decoded(dev, t, x, y, p, [0, n]), TM, h, w).cpu().numpy()
    ti = t.astype(np.int64)
    win = (ti[-1] - ti[0]) // TM
    k = (ti - ti[0]) // win
    keep = k < TM
    want = np.zeros((1, TM, 2, h, w), dtype=np.int32)
    np.add.at(want[0], (k[keep], (p[keep] != 0).astype(np.int64), y[keep].astype(np.int64), x[keep].astype(np.int64)), 1)
    assert np.array_equal(counts, want) and want[0, :, 1].sum() > odd[keep].sum()
    surf = ops.event_time_surface(*decoded(dev, t, x, y, p, [0, n]), TM, h, w)
    m = ~odd
    without = ops.event_time_surface(*decoded(dev, t[m], x[m], y[m], p[m], [0, int(m.sum())]), TM, h, w)
    assert torch.equal(surf, without) and (surf > 0).all()
    binary = ops.event_time_surface(*decoded(dev, t, x, y, np.minimum(p, 1), [0, n]), TM, h, w)
    assert not torch.equal(surf, binary)                                    # the odd events would have shown


def test_window_of_zero_length_gives_zeros_and_leaves_the_neighbour_alone(dev):
    h, w = 24, 32
    t0, x0, y0, p0 = events_ref.synth_events(1500, h, w, seed=11)
    t1, x1, y1, p1 = events_ref.synth_events(400, h, w, seed=12)
    t1 = np.full_like(t1, 1_234_567)                                        # every event on one timestamp
    t, x, y, p = (np.concatenate(v) for v in ((t1, t0), (x1, x0), (y1, y0), (p1, p0)))
    offsets = [0, 400, 1900]
    rec = torch.from_numpy(dat_records(t, x, y, p, h, w)).to(dev)
    ranges = torch.tensor([[0, 400], [400, 1900]], dtype=torch.int64, device=dev)
    counts = ops.event_histogram_dat_ranges(rec, ranges, TM, h, w)
    latest = ops.event_latest_surface_dat_ranges(rec, ranges, TM, h, w)
    surf = ops.event_time_surface(*decoded(dev, t, x, y, p, offsets), TM, h, w)
    for got in (counts, latest, surf):
        assert not got[0].any() and got[1].any()
    assert torch.equal(latest, surf)
    alone = decoded(dev, t0, x0, y0, p0, [0, 1500])
    assert torch.equal(counts[1:], ops.event_histogram(*alone, TM, h, w))
    assert torch.equal(surf[1:], ops.event_time_surface(*alone, TM, h, w))
    assert torch.equal(latest[1:], ops.event_latest_surface_dat_ranges(rec, ranges[1:], TM, h, w))


def test_atis_count_and_latest_entries_report_the_same_oob_and_flags(dev):
    """two recordings, Tl = 2: a plain one with events outside the (smaller) sensor, and one whose times decrease once (flag bit 0)"""
    h, w = 36, 48
    first, _ = data.synth_atis_batch(1, 3000, h, w, span_us=100_000, seed=3)
    rng = np.random.default_rng(4)
    t = np.sort(rng.integers(0, 60_000, size=500))
    t[[200, 201]] = t[[201, 200]] + np.array([1, 0])
    second = data.encode_atis(t, rng.integers(0, w, size=500), rng.integers(0, h, size=500), rng.integers(0, 2, size=500))
    rec = torch.from_numpy(np.concatenate([first, second])).to(dev)
    off = torch.tensor([0, len(first) // 5, (len(first) + len(second)) // 5], dtype=torch.int64, device=dev)
    _, c_oob, c_flags = ops.event_histogram_atis(rec, off, 2, TM, h - 4, w - 5, return_oob=True, return_flags=True)
    _, l_oob, l_flags = ops.event_latest_surface_atis(rec, off, 2, TM, h - 4, w - 5, return_oob=True, return_flags=True)
    assert torch.equal(l_oob, c_oob) and (c_oob > 0).all()
    assert torch.equal(l_flags & 3, c_flags & 3) and c_flags.tolist() == [0, 1]
