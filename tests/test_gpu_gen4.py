"""GPU tests of the 1 Mpx front end: ``ops.stacked_hist_frames`` against the fixture recorded from the reference's generate_slices
(tests/golden/stacked_hist.npz), against the numpy checker (tests/gen4_ref.py, pinned to that fixture by test_cpu_gen4.py) on every path of
the kernel, against the two existing kernels it must agree with bit for bit, and the loader / ``data.rvt_to_frames`` eagerly and replayed
from a captured graph.  Bin sums are integers and the resize is contraction-free float64 arithmetic with float32 weights, so every
comparison is exact."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

import gen4_ref
from eas_snn_amd import _lib, data, ops

pytestmark = pytest.mark.gpu

# (nw, nh, dx, dy, flip) on the 18 x 32 sensor and the 32 x 48 canvas, one kernel path each
RESIZE_ROWS = [(32, 18, 0, 0, 0),        # copy
               (32, 18, 9, 7, 1),        # copy, shifted and flipped
               (20, 11, 5, 3, 0),        # downscale: some source rows are never read
               (13, 7, 30, 20, 1),       # strong downscale at the canvas corner
               (48, 27, 0, 2, 0),        # upscale
               (40, 32, 8, 0, 1)]        # upscale beyond the sensor in both axes


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


def i64(v, dev):
    return torch.tensor(list(v), dtype=torch.int64, device=dev)


def run(dev, store, first, Tm, Hc, Wc, nbins, lo=None, params=None):
    out, flags = ops.stacked_hist_frames(torch.from_numpy(store).to(dev), i64(first, dev), Tm, Hc, Wc, nbins=nbins,
                                         lo=None if lo is None else i64(lo, dev),
                                         params=None if params is None else torch.tensor(params, dtype=torch.int32, device=dev),
                                         return_flags=True)
    assert out.shape == (len(first), 1, Tm, 2, Hc, Wc) and out.dtype == torch.float32 and flags.shape == (len(first),)
    return out.cpu().numpy(), flags.cpu().numpy()


def test_golden_bit_exact(dev):
    """every geometry of the fixture as a store, all its cases as batches through ``first`` (one call per slice count), params None"""
    g = load_golden('stacked_hist')
    cases = {}
    for key in [str(k) for k in g['cases']]:
        name, spec = key.split('/')
        cases.setdefault(name, []).append((int(spec[1:spec.index('_')]), int(spec[spec.index('_n') + 2:]), g[key]))
    assert sorted(cases) == ['bins3', 'ragged_w', 'saturated', 'small']
    for name, rows in cases.items():
        store = g[f'{name}/data']
        R, nb2, H, W = store.shape
        Hc, Wc = (H + 31) // 32 * 32, (W + 31) // 32 * 32
        obj2repr = np.arange(R)
        for Tm in sorted({n for _, n, _ in rows}):
            batch = [(t, want) for t, n, want in rows if n == Tm]
            first = [int(data.rvt_first_index(obj2repr, t, Tm)) for t, _ in batch]
            out, flags = run(dev, store, first, Tm, Hc, Wc, nb2 // 2)
            assert not flags.any()
            for b, (t, want) in enumerate(batch):
                assert np.array_equal(out[b, :, :, :, :H, :W].astype(np.float64), want), (name, t, Tm)
                assert out[b].sum(dtype=np.float64) == want.sum(), (name, t, Tm, 'padding is not zero')
    assert g['saturated/t5_n4'].max() == 2550.0            # sums beyond 8 bits are in the fixture


def small_store(W=32, nbins=10, seed=0):
    """R = 7 representations of an 18-row sensor: two recordings back to back, representations 0-3 and 4-6"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (7, 2 * nbins, 18, W), dtype=np.uint8)


def test_stores_and_bounds(dev):
    store = small_store()
    first, lo = [-2, 3, 4, 5, 1, 0], [0, 4, 4, 4, 0, 0]
    want, want_flags = gen4_ref.frames(store, first, 3, 18, 32, lo=lo)
    out, flags = run(dev, store, first, 3, 18, 32, 10, lo=lo)
    assert np.array_equal(out, want)
    assert list(flags) == [0, 0, 0, 1, 0, 0] and np.array_equal(flags, want_flags.astype(flags.dtype))
    assert not out[0, 0, :2].any() and out[0, 0, 2].any()                  # two zero slices in front
    assert not out[1, 0, 0].any() and out[1, 0, 1].any()                   # index 3 belongs to the neighbour recording
    assert all(out[2, 0, j].any() for j in range(3))
    assert not out[3, 0, 2].any() and out[3, 0, 1].any()                   # index 7 >= R
    # slices that must not be read hold a sentinel: the result does not move
    marked = store.copy()
    marked[3] = 255                                                         # below lo = 4 for samples 1-3, behind sample 0's slices
    out2, _ = run(dev, marked, first[:4], 3, 18, 32, 10, lo=lo[:4])
    assert np.array_equal(out2, out[:4])
    # lo = None is 0 for every sample; indices far outside on both sides are zero slices
    out3, flags3 = run(dev, store, [-2, 6, -10 ** 15, 10 ** 15, 2 ** 63 - 1, -2 ** 63], 3, 18, 32, 10)
    want3, wf3 = gen4_ref.frames(store, [-2, 6, -10 ** 15, 10 ** 15, 2 ** 63 - 1, -2 ** 63], 3, 18, 32)
    assert np.array_equal(out3, want3) and list(flags3) == [0, 1, 0, 1, 1, 0] == list(wf3)


@pytest.mark.parametrize('W,nbins', [(32, 10), (30, 10), (32, 3)], ids=['w32', 'w30_bytes', 'bins3_generic'])
def test_resize_paths(dev, W, nbins):
    store = small_store(W, nbins, seed=W + nbins)
    Hc, Wc, Tm = 32, 48, 3
    rows = [(W, 18, 0, 0, 0), (W, 18, 9, 7, 1)] + RESIZE_ROWS[2:]         # the copy path is the sensor's own size
    first = [4, 1, 0, 2, -1, 3]
    want, _ = gen4_ref.frames(store, first, Tm, Hc, Wc, nbins=nbins, params=rows)
    out, flags = run(dev, store, first, Tm, Hc, Wc, nbins, params=rows)
    for b, row in enumerate(rows):
        assert np.array_equal(out[b], want[b]), (row, int((out[b] != want[b]).sum()))
    assert not flags.any() and out.any()

    # a downscale names only some source rows: what the others hold does not matter.  (At 11 of 18 rows every source row is still some
    # tap's -- two taps per output row cover a scale below 2 --; at 7 of 18 four rows are nobody's.)
    for k, least in ((2, 0), (3, 3)):
        nh = rows[k][1]
        named = set()
        for j in range(nh):
            s = min(max(int(np.floor(np.float32((j + 0.5) * (18 / nh) - 0.5))), 0), 17)
            named |= {s, min(s + 1, 17)}
        unread = sorted(set(range(18)) - named)
        assert len(unread) >= least
        base, _ = run(dev, store, [1], Tm, Hc, Wc, nbins, params=[rows[k]])
        assert np.array_equal(base, gen4_ref.frames(store, [1], Tm, Hc, Wc, nbins=nbins, params=[rows[k]])[0]) and base.any()
        for fill in (255, 0):
            changed = store.copy()
            changed[:, :, unread, :] = fill
            again, _ = run(dev, changed, [1], Tm, Hc, Wc, nbins, params=[rows[k]])
            assert np.array_equal(again, base), (rows[k], fill)

    # an empty rectangle is a zero canvas; a rectangle that sticks out of the canvas is clipped (a defined input: the kernel is a
    # bounds-checked gather per output pixel)
    odd = [(0, 11, 5, 3, 0), (20, 0, 5, 3, 1), (-7, -7, 0, 0, 0), (20, 11, 40, 28, 0), (20, 11, 40, 28, 1), (W, 18, -5, -4, 0), (40, 32, -9, 20, 1),
           (20, 11, 48, 0, 0), (20, 11, 0, -11, 0)]
    first = [2] * len(odd)
    want, _ = gen4_ref.frames(store, first, Tm, Hc, Wc, nbins=nbins, params=odd)
    out, _ = run(dev, store, first, Tm, Hc, Wc, nbins, params=odd)
    for b, row in enumerate(odd):
        assert np.array_equal(out[b], want[b]), row
    assert not out[0].any() and not out[1].any() and not out[2].any() and not out[7].any() and not out[8].any()
    assert out[3].any() and out[3][..., :28, :].sum() == 0 and out[3][..., :40].sum() == 0


def test_canvas_smaller_than_the_sensor(dev):
    """geometry is not restricted to Hc >= H, Wc >= W: the training canvas is the model input"""
    store = small_store(48, 10, seed=9)
    rows = [(16, 9, 0, 0, 0), (48, 18, 0, 0, 0), (48, 18, -20, -5, 1), (30, 12, -8, 2, 0)]
    want, _ = gen4_ref.frames(store, [0, 1, 2, 3], 2, 12, 16, params=rows)
    out, _ = run(dev, store, [0, 1, 2, 3], 2, 12, 16, 10, params=rows)
    assert np.array_equal(out, want) and out[1].any()


def test_same_as_the_two_existing_kernels(dev):
    """config-4 geometry: equal to ``counts_letterbox`` of the int32 bin sums, and with params None to ``stacked_hist_event_sum``"""
    B, Tm, R, H, W, Hc, Wc = 4, 4, 16, 360, 640, 384, 640
    g = torch.Generator().manual_seed(3)
    store = torch.poisson(torch.full((R, 20, H, W), 0.3), generator=g).clamp_(max=255).to(torch.uint8)
    store[5] = 255                                                          # sums of 2550 at full size
    store = store.to(dev)
    first = torch.tensor([12, 2, 5, 9], dtype=torch.int64, device=dev)
    rows = [data.letterbox_params(H, W, Hc, Wc),                            # (640, 360, 0, 0, 0)
            (W, H, 0, 0, 0),
            (301, 163, 211, 97, 1),                                         # jitter rows, written out: scale 0.47 flipped, scale 0.93
            (597, 371, 17, 9, 0)]
    assert rows[0] == (640, 360, 0, 0, 0)
    params = torch.tensor(rows, dtype=torch.int32, device=dev)
    gathered = torch.stack([store[int(f):int(f) + Tm] for f in first.tolist()])                   # [B, Tm, 20, H, W]
    sums = gathered.view(B, Tm, 2, 10, H, W).to(torch.int32).sum(3).to(torch.int32).contiguous()
    assert int(sums.max()) == 2550
    want = ops.counts_letterbox(sums, params, Hc, Wc).unsqueeze(1)
    got = ops.stacked_hist_frames(store, first, Tm, Hc, Wc, params=params)
    assert got.shape == want.shape == (B, 1, Tm, 2, Hc, Wc)
    assert torch.equal(got, want), int((got != want).sum())
    plain = ops.stacked_hist_frames(store, first, Tm, Hc, Wc)
    assert torch.equal(plain, ops.stacked_hist_event_sum(gathered, Hc, Wc))
    assert torch.equal(plain[:2], got[:2])                                  # the letterbox row and the identity are params None


def test_bands_shorter_than_eight_rows(dev):
    """a 1280-pixel sensor: 8 output rows per block (16 staged rows + the column table) do not fit the kernel's 48 KiB of LDS, bands are 4
    rows; the 11-row canvas takes three, the last one of 3 rows.  Both entry points."""
    from oracle import events_ref
    assert 2 * 8 * 1280 * 2 + 1280 * 8 > 48 * 1024 >= 2 * 4 * 1280 * 2 + 1280 * 8
    store = np.random.default_rng(12).integers(0, 256, (2, 6, 10, 1280), dtype=np.uint8)
    Hc, Wc = 11, 1280
    for rows in (None, [(900, 7, 100, 2, 1), (1280, 10, 0, 0, 0)], [(1100, 9, 700, 5, 0), (640, 5, -300, -2, 1)]):
        want, _ = gen4_ref.frames(store, [0, 1], 1, Hc, Wc, nbins=3, params=rows)
        out, flags = run(dev, store, [0, 1], 1, Hc, Wc, 3, params=rows)
        assert np.array_equal(out, want) and out[0].any() and out[1].any() and not flags.any(), rows
    got = ops.stacked_hist_event_sum(torch.from_numpy(store).to(dev).view(2, 1, 6, 10, 1280), Hc, Wc, nbins=3).cpu().numpy()
    for b in range(2):
        want = events_ref.pad_to_canvas(events_ref.stacked_hist_event_sum(store[b:b + 1], 1, 10, 1280), Hc, Wc)
        assert np.array_equal(got[b].astype(np.float64), want)
    assert got[..., :10, :].any() and not got[..., 10:, :].any()


def small_exp():
    return types.SimpleNamespace(Tm=3, input_size=(32, 48), num_classes=3)


def test_loader_frames_and_targets(dev):
    exp = small_exp()
    loader = data.SyntheticStackedHistLoader(exp, batch_size=4, representations=9, sensor_hw=(18, 32), rate=0.3, seed=2)
    assert len(loader) == 2
    draws = loader.batches(0)
    seen = np.concatenate([d[0] for d in draws])
    assert draws[0][1].shape == (4, 5) and len(set(seen.tolist())) == 8 and seen.min() >= 0 and seen.max() < 9          # part of a permutation
    store = loader.store(dev).cpu().numpy()
    assert store.shape == (9, 20, 18, 32) and store.any()
    n = 0
    for (frames, targets), (idx, par) in zip(loader, draws):
        assert frames.shape == (4, 1, 3, 2, 32, 48) and frames.dtype == torch.float32 and frames.is_cuda
        assert targets.shape == (4, 50, 5) and targets.dtype == torch.float32 and targets.is_cuda
        first = data.rvt_first_index(np.arange(9), idx, 3)
        want, _ = gen4_ref.frames(store, first, 3, 32, 48, params=par)
        assert np.array_equal(frames.cpu().numpy(), want)
        t = targets.cpu().numpy()
        for b in range(4):
            box = data.transform_boxes(loader.raw_boxes(idx[b]), tuple(int(v) for v in par[b]), 18, 32, 32, 48)
            assert np.array_equal(t[b, :len(box), 0], box[:, 4])
            assert np.array_equal(t[b, :len(box), 1:], np.stack([(box[:, 0] + box[:, 2]) / 2, (box[:, 1] + box[:, 3]) / 2, box[:, 2] - box[:, 0],
                                                                 box[:, 3] - box[:, 1]], axis=-1))
            assert not t[b, len(box):].any()
        n += 1
    assert n == 2 and loader.epoch == 1
    assert not np.array_equal(loader.batches(1)[0][0], draws[0][0]) or not np.array_equal(loader.batches(1)[0][1], draws[0][1])
    # the experiment hands this loader out only when asked to
    from yolox.exp import get_exp
    e = get_exp(None, 'e-yolox-s')
    assert type(e.get_data_loader(4, False)).__name__ == 'SyntheticEventLoader'
    e.train_input = 'stacked_hist'
    assert isinstance(e.get_data_loader(4, False), data.SyntheticStackedHistLoader)


def test_rvt_to_frames_replays_from_a_captured_graph(dev):
    exp = small_exp()
    store_np = small_store(seed=4)
    store = torch.from_numpy(store_np).to(dev)
    obj2repr = torch.arange(7, device=dev)
    labels = torch.tensor([0, 6, 3, 5], device=dev)
    lo = torch.tensor([0, 4, 0, 4], device=dev)
    rows = [RESIZE_ROWS[2], RESIZE_ROWS[1], RESIZE_ROWS[4], RESIZE_ROWS[3]]
    params = torch.tensor(rows, dtype=torch.int32, device=dev)

    def chain():
        return data.rvt_to_frames(store, data.rvt_first_index(obj2repr, labels, exp.Tm), exp, params, lo=lo)
    eager = chain()
    want, _ = gen4_ref.frames(store_np, [-2, 4, 1, 3], 3, 32, 48, lo=[0, 4, 0, 4], params=rows)
    assert np.array_equal(eager.cpu().numpy(), want)
    side = _lib.private_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                             # allocator warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = chain()                                                   # no host read inside: the capture would fail
    torch.cuda.current_stream().wait_stream(side)
    # new labels and draws in the captured tensors: the replay follows them
    labels.copy_(torch.tensor([2, 4, 6, 1], device=dev))
    params.copy_(torch.tensor(rows[::-1], dtype=torch.int32, device=dev))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want2, _ = gen4_ref.frames(store_np, [0, 2, 4, -1], 3, 32, 48, lo=[0, 4, 0, 4], params=rows[::-1])
    assert np.array_equal(out.cpu().numpy(), want2)
    # numpy rows work too (copied to the device by the call)
    assert torch.equal(data.rvt_to_frames(store, torch.tensor([0, 2, 4, -1], device=dev), (3, (32, 48)), rows[::-1], lo=lo), out)
