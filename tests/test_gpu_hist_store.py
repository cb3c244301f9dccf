"""GPU tests of 1 Mpx training from recordings in HBM: ``ops.stacked_hist_bin_sums`` against the reference's reshape-and-sum on every path of
the kernel; ``ops.count_store_frames`` against ``ops.stacked_hist_frames`` on the unsummed store and against the numpy checker
(tests/gen4_ref.py) at the shapes where the band kernel can go wrong; ``data.Gen4Store`` built chunk by chunk from the recordings of
tests/golden/gen4_store.npz against the slices and boxes the reference made of them; the loaders, eagerly and replayed from a captured
graph; the experiment's ``train_input = 'hist_store'``, a short Trainer run and the Prophesee-protocol evaluation.  Every value is an
integer below 2^24 or the result of the one arithmetic both sides share, so every comparison is exact.

The Trainer run uses a 64 x 96 canvas, not 32 x 48: the model's canvas has to be a multiple of 32 in both axes (its stride-32 level is
upsampled by 2 and concatenated with the stride-16 level, which at 32 x 48 would be 2 x 4 against 2 x 3), so 64 x 96 is the smallest canvas
of that aspect the model takes; the loaders themselves are tested at 32 x 48."""
import types
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

import gen4_ref
import gen4_store_ref
from eas_snn_amd import _lib, data, ops

pytestmark = pytest.mark.gpu

RESIZE_ROWS = [(20, 11, 5, 3, 0),        # downscale: some source rows are never read
               (13, 7, 30, 20, 1),       # strong downscale at the canvas corner, flipped
               (48, 27, 0, 2, 0),        # upscale
               (40, 32, 8, 0, 1),        # upscale beyond the sensor in both axes
               (20, 11, 40, 28, 1),      # sticks out of the canvas
               (0, 11, 5, 3, 0),         # an empty rectangle
               (20, 11, 48, 0, 0)]       # off the canvas


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


def i64(v, dev):
    return torch.tensor(list(v), dtype=torch.int64, device=dev)


# ------------------------------------------------------------------------------------------------ the builder
@pytest.mark.parametrize('H,W,nbins', [(18, 32, 10), (18, 30, 10), (18, 32, 3), (5, 40, 10)], ids=['vector', 'bytes', 'bins3_generic', 'w40_bytes'])
def test_bin_sums(dev, H, W, nbins):
    rng = np.random.default_rng(H * W + nbins)
    hist = rng.integers(0, 256, (5, 2 * nbins, H, W), dtype=np.uint8)
    hist[2, :, 7 % H, W - 1] = 255                                            # 255 in every bin of one pixel, both polarities
    want = gen4_store_ref.bin_sums(hist, nbins)
    assert want[2, 0, 7 % H, W - 1] == 255 * nbins
    got = ops.stacked_hist_bin_sums(torch.from_numpy(hist).to(dev), nbins)
    assert got.dtype == torch.uint16 and got.shape == (5, 2, H, W) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    # into a view at a non-zero offset of a store allocated once: the neighbours stay as they were
    store = torch.full((9, 2, H, W), 0xABCD, dtype=torch.uint16, device=dev)
    out = ops.stacked_hist_bin_sums(torch.from_numpy(hist[1:4]).to(dev), nbins, out=store[3:6])
    assert out.data_ptr() == store[3:6].data_ptr()
    s = store.cpu().numpy()
    assert np.array_equal(s[3:6], want[1:4]) and (s[:3] == 0xABCD).all() and (s[6:] == 0xABCD).all()
    # n = 0: no launch, shapes kept
    empty = ops.stacked_hist_bin_sums(torch.zeros((0, 2 * nbins, H, W), dtype=torch.uint8, device=dev), nbins)
    assert empty.shape == (0, 2, H, W) and empty.dtype == torch.uint16
    ops.stacked_hist_bin_sums(torch.zeros((0, 2 * nbins, H, W), dtype=torch.uint8, device=dev), nbins, out=store[4:4])
    assert np.array_equal(store.cpu().numpy(), s)


def test_bin_sums_largest_sum(dev):
    """nbins = 255 on a 2 x 16 map, every bin of one pixel at 255: 65 025, the largest sum sixteen bits have to hold"""
    hist = np.random.default_rng(1).integers(0, 256, (2, 510, 2, 16), dtype=np.uint8)
    hist[1, 255:, 1, 15] = 255
    hist[0, :255, 0, 0] = 255
    got = ops.stacked_hist_bin_sums(torch.from_numpy(hist).to(dev), 255).cpu().numpy()
    assert np.array_equal(got, gen4_store_ref.bin_sums(hist, 255)) and got[1, 1, 1, 15] == 65025 and got[0, 0, 0, 0] == 65025
    with pytest.raises(_lib.EasHipError):
        ops.stacked_hist_bin_sums(torch.zeros((1, 512, 2, 16), dtype=torch.uint8, device=dev), 256)


# ------------------------------------------------------------------------------------------------ frames from the summed store
def both(dev, store, first, Tm, Hc, Wc, nbins, lo=None, params=None):
    """``count_store_frames`` on the sums of ``store``; asserts that frames and flags equal ``stacked_hist_frames`` on ``store`` itself and the
    checker on ``store``, returns (frames, flags) as numpy arrays"""
    st = torch.from_numpy(store).to(dev)
    sums = ops.stacked_hist_bin_sums(st, nbins)
    kw = dict(lo=None if lo is None else i64(lo, dev), params=None if params is None else torch.tensor(params, dtype=torch.int32, device=dev),
              return_flags=True)
    out, flags = ops.count_store_frames(sums, i64(first, dev), Tm, Hc, Wc, **kw)
    ref, ref_flags = ops.stacked_hist_frames(st, i64(first, dev), Tm, Hc, Wc, nbins=nbins, **kw)
    assert out.shape == (len(first), 1, Tm, 2, Hc, Wc) and out.dtype == torch.float32 and flags.shape == (len(first),) and flags.dtype == torch.int32
    assert torch.equal(out, ref) and torch.equal(flags, ref_flags)
    want, want_flags = gen4_ref.frames(store, first, Tm, Hc, Wc, nbins=nbins, lo=lo, params=params)
    out, flags = out.cpu().numpy(), flags.cpu().numpy()
    assert np.array_equal(out, want) and np.array_equal(flags, want_flags.astype(flags.dtype))
    return out, flags


def small_store(W=32, nbins=10, seed=0):
    """R = 7 representations of an 18-row sensor: two recordings back to back, representations 0-3 and 4-6"""
    return np.random.default_rng(seed).integers(0, 256, (7, 2 * nbins, 18, W), dtype=np.uint8)


def test_frames_indices_and_bounds(dev):
    store = small_store()
    first, lo = [-2, 3, 4, 5, 1, 0, 7], [0, 4, 4, 4, 0, 0, 4]
    out, flags = both(dev, store, first, 3, 18, 32, 10, lo=lo)
    assert list(flags) == [0, 0, 0, 1, 0, 0, 1]
    assert not out[0, 0, :2].any() and out[0, 0, 2].any()                  # two zero slices in front
    assert not out[1, 0, 0].any() and out[1, 0, 1].any()                   # index 3 belongs to the neighbour recording
    assert not out[3, 0, 2].any() and out[3, 0, 1].any() and not out[6].any()        # index 7 = R and behind it
    far = [-2, 6, -10 ** 15, 10 ** 15, 2 ** 63 - 1, -2 ** 63]
    out, flags = both(dev, store, far, 3, 18, 32, 10)
    assert list(flags) == [0, 1, 0, 1, 1, 0] and not out[2:].any()


@pytest.mark.parametrize('W,nbins', [(32, 10), (30, 10), (40, 3)], ids=['w32', 'w30_elements', 'w40_half_group'])
def test_frames_resize_paths(dev, W, nbins):
    """16-byte row copies (W % 8 == 0, with a last group of 8 pixels at W = 40) and the element path, under copies, jittered, flipped,
    clipped, empty and off-canvas rows and under params None"""
    store = small_store(W, nbins, seed=W + nbins)
    rows = [(W, 18, 0, 0, 0), (W, 18, 9, 7, 1), (W, 18, -5, -4, 0)] + RESIZE_ROWS
    first = [4, 1, 0, 2, -1, 3, 2, 2, 2, 2]
    out, flags = both(dev, store, first, 3, 32, 48, nbins, lo=[4, 0, 0, 0, 0, 0, 0, 0, 0, 0], params=rows)
    assert not flags.any() and all(out[b].any() for b in range(7)) and not out[8].any() and not out[9].any()
    plain, _ = both(dev, store, [1, 5], 3, 32, 48, nbins)
    assert plain[0, 0, :, :, :18, :W].any() and not plain[0, 0, :, :, 18:].any() and not plain[0, 0, :, :, :, W:].any()


def test_frames_canvas_smaller_than_the_sensor(dev):
    store = small_store(48, 10, seed=9)
    rows = [(16, 9, 0, 0, 0), (48, 18, 0, 0, 0), (48, 18, -20, -5, 1), (30, 12, -8, 2, 0)]
    out, _ = both(dev, store, [0, 1, 2, 3], 2, 12, 16, 10, params=rows)
    assert out[1].any()


def test_frames_bands_shorter_than_eight_rows(dev):
    """a 1280-pixel sensor: bands of 4 rows (``frames_band_rows``); two samples, the 11-row canvas takes three bands"""
    assert 2 * 8 * 1280 * 2 + 1280 * 8 > 48 * 1024 >= 2 * 4 * 1280 * 2 + 1280 * 8
    store = np.random.default_rng(12).integers(0, 256, (2, 6, 10, 1280), dtype=np.uint8)
    for rows in (None, [(900, 7, 100, 2, 1), (1280, 10, 0, 0, 0)], [(1100, 9, 700, 5, 0), (640, 5, -300, -2, 1)]):
        out, flags = both(dev, store, [0, 1], 1, 11, 1280, 3, params=rows)
        assert out[0].any() and out[1].any() and not flags.any(), rows


# ------------------------------------------------------------------------------------------------ the store
@pytest.fixture(scope='module')
def golden():
    return load_golden('gen4_store')


@pytest.fixture(scope='module')
def recordings(golden):
    return gen4_store_ref.fixture_recordings(golden)


@pytest.fixture(scope='module')
def store(dev, recordings):
    """chunks of 2 representations: the seams fall inside both recordings (7 and 5 representations)"""
    return data.Gen4Store(recordings, 3, dev, sensor_hw=(12, 16), chunk=2)


@pytest.fixture(scope='module')
def tab(recordings):
    return gen4_store_ref.tables(recordings, 3, 2, (12, 16))


def small_exp():
    return types.SimpleNamespace(Tm=3, Tl=1, input_size=(32, 48), test_size=(32, 48), num_classes=3)


def test_store_equals_the_reference_fixture(dev, golden, recordings, store, tab):
    assert store.sums.dtype == torch.uint16 and store.sums.shape == (12, 2, 12, 16) and store.sums.is_cuda and store.boxes.is_cuda
    assert np.array_equal(store.sums.cpu().numpy(), np.concatenate([gen4_store_ref.bin_sums(r[1]) for r in recordings]))
    for k in ('rep_offsets', 'group_first', 'group_lo', 'boxes', 'group_start'):
        assert np.array_equal(getattr(store, k).cpu().numpy(), tab[k]), k
    exp = small_exp()
    idx = torch.arange(7, device=dev)
    for params in (None, data.unscaled_params(7, (12, 16), dev), [(16, 12, 0, 0, 0)] * 7):
        got = store.frames(idx, params, exp).cpu().numpy()
        assert got.shape == (7, 1, 3, 2, 32, 48)
        assert np.array_equal(got[..., :12, :16].astype(np.float64), golden['slices'][:, 0][:, None])
        assert got.sum(dtype=np.float64) == golden['slices'].sum()                # zero padded to the canvas
    assert np.array_equal(store.frames(idx, None, exp, canvas_hw=(12, 16)).cpu().numpy().astype(np.float64), golden['slices'][:, 0][:, None])
    # targets under drawn params and permutations, the sample without boxes included
    rs = np.random.RandomState(5)
    ids = np.array([1, 0, 5, 3, 2, 6, 4, 1], dtype=np.int64)
    par = np.array([data.jitter_params(12, 16, 32, 48, jitter=.3, rng=rs) for _ in ids], dtype=np.int32)
    perm = np.tile(np.arange(3, dtype=np.int32), (len(ids), 1))
    for b, s in enumerate(ids):
        perm[b, :store.group_rows[s]] = rs.permutation(int(store.group_rows[s]))
    t, count, flags = store.targets(torch.from_numpy(ids).to(dev), par, torch.from_numpy(perm).to(dev), (32, 48), return_info=True)
    want = gen4_store_ref.targets(tab, ids, par, (12, 16), (32, 48), perm=perm)
    assert np.array_equal(t.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1]) and not flags.any().item()
    assert not t[0].any().item() and not t[7].any().item() and t.shape == (8, 50, 5) and want[1].sum() > 0
    got = store.frames(torch.from_numpy(ids).to(dev), par, exp).cpu().numpy()
    assert np.array_equal(got, gen4_store_ref.frames(recordings, tab, ids, 3, 32, 48, params=par)) and got.any()


def test_loader_step_equals_the_checker(dev, recordings, store, tab):
    exp = small_exp()
    loader = data.Gen4StoreLoader(exp, 2, store=store, seed=2)
    draws = loader.batches(0)
    assert len(loader) == 3 and len(draws) == 3
    n = 0
    for (frames, targets), (idx, par, perm) in zip(loader, draws):
        assert frames.shape == (2, 1, 3, 2, 32, 48) and frames.dtype == torch.float32 and frames.device == dev
        assert targets.shape == (2, 50, 5) and targets.dtype == torch.float32 and targets.device == dev
        assert np.array_equal(frames.cpu().numpy(), gen4_store_ref.frames(recordings, tab, idx, 3, 32, 48, params=par))
        want, _, flags = gen4_store_ref.targets(tab, idx, par, (12, 16), (32, 48), perm=perm)
        assert np.array_equal(targets.cpu().numpy(), want) and not flags.any()
        n += 1
    assert n == 3 and loader.epoch == 1


def test_eval_loader_yields_the_evaluation_tuple(dev, recordings, store, tab):
    from yolox.evaluators.psee_evaluator import time_from_name
    exp = small_exp()
    loader = data.Gen4StoreEvalLoader(exp, 4, [0, 5, 1, 2, 6, 3], store)
    assert len(loader) == 2 and loader.dataset.sample_names is store.sample_names and loader.dataset.map_val and not loader.dataset.random_aug
    assert loader.dataset.class_names == ['0', '1', '2'] and len(loader.dataset) == 7
    times = [int(r[5][k]) for r in recordings for k in range(len(r[5]))]
    assert [time_from_name(n) for n in store.sample_names] == times
    row = data.letterbox_params(12, 16, 32, 48)
    for (frames, labels, (hs, ws), ids), want_ids in zip(loader, ([0, 5, 1, 2], [6, 3])):
        assert ids.tolist() == want_ids and hs.tolist() == [12] * len(want_ids) and ws.tolist() == [16] * len(want_ids)
        want = gen4_store_ref.frames(recordings, tab, want_ids, 3, 32, 48, params=[row] * len(want_ids))
        assert np.array_equal(frames.cpu().numpy(), want) and frames.shape[0] == len(want_ids)
        for i, lab in zip(want_ids, labels):
            assert lab.dtype == torch.float32 and not lab.is_cuda and np.array_equal(lab.numpy(), store.raw_labels(i)) and lab.shape[1] == 5


def test_frames_replay_from_a_captured_graph(dev, recordings, store, tab):
    exp = small_exp()
    loader = data.Gen4StoreLoader(exp, 2, store=store, seed=5)
    (i0, p0, _), (i1, p1, _) = loader.batches(0)[:2]
    idx, par = torch.from_numpy(i0).to(dev), torch.from_numpy(p0).to(dev)

    def chain():
        return store.frames(idx, par, exp)
    side = _lib.private_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                             # allocator warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            frames = chain()                                                # no host read inside: the capture would fail
    torch.cuda.current_stream().wait_stream(side)
    idx.copy_(torch.from_numpy(i1))                                         # new indices and draws in the captured tensors
    par.copy_(torch.from_numpy(p1))
    frames.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(frames.cpu().numpy(), gen4_store_ref.frames(recordings, tab, i1, 3, 32, 48, params=p1))
    assert not np.array_equal(i0, i1) and torch.equal(frames, chain())


# ------------------------------------------------------------------------------------------------ the experiment
BASE_OPTS = ['T', '3', 'embedding', 'arsnn', 'num_classes', '3', 'spike_attach', 'True', 'thresh', '1', 'readout', 'sum', 'embedding_depth', '2',
             'embedding_ksize', '5', 'write_zero', 'True', 'spike_fn', 'atan', 'use_spike', 'True', 'input_size', '(64, 96)', 'test_size', '(64, 96)']


def test_trainer_and_prophesee_evaluation_on_the_store_loaders(dev, tmp_path, monkeypatch):
    """two iterations of ``yolox.core.Trainer.train()`` fed by ``train_input = 'hist_store'`` at 64 x 96 (module docstring), batch 2, with
    finite losses; then ``get_evaluator`` with ``eval_proph``: a PSEEEvaluator for the downsampled 1 Mpx camera, without the warning, that
    evaluates the synthetic test store with the detections left on the device (``last_match``)"""
    from oracle import fill
    from yolox.evaluators.psee_evaluator import PSEEEvaluator
    from yolox.exp import get_exp
    monkeypatch.setattr(ops, 'VERIFY_SMALL_INT', False)      # the suite's tag check reads the device: not inside a capture
    exp = get_exp(None, 'e-yolox-s')
    exp.merge(BASE_OPTS + ['test_conf', '0.00003', 'nmsthre', '0.5', 'data_name', 'gen4', 'eval_proph', 'True'])
    exp.max_epoch, exp.print_interval, exp.output_dir = 1, 1, str(tmp_path)
    exp.train_input, exp.store_recordings = 'hist_store', (1, 8)                # 5 object frames: two batches of 2
    torch.manual_seed(5)
    tr = exp.get_trainer(types.SimpleNamespace(batch_size=2, fp16=False, experiment_name='hist_store', ckpt=None, resume=False))
    tr.train()
    assert isinstance(tr.train_loader, data.Gen4StoreLoader) and len(tr.train_loader) == 2 and tr.train_loader.store.sensor_hw == (64, 96)
    assert len(tr.log) == 2 and all(np.isfinite(r['loss']) for r in tr.log)
    torch.cuda.set_stream(torch.cuda.default_stream())
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        evaluator = exp.get_evaluator(2, False)
    assert type(evaluator) is PSEEEvaluator and evaluator.evaluator.dataset == 'gen4' and evaluator.evaluator.downsample_by_2 is True
    assert isinstance(evaluator.dataloader, data.Gen4StoreEvalLoader) and evaluator.dataloader.store is not tr.train_loader.store
    model = exp.get_model()
    fill.procedural_fill_(model, 2.0, ann_regex=fill.ANN_KEYS['True'])
    model.to(dev).eval()
    evaluator.evaluate(model, False, False, None, None, exp.test_size)
    assert evaluator.last_match is not None and set(evaluator.last_match) == {'images', 'detections', 'ground_truths'}
