"""GPU tests of N-Caltech101 training from recordings in HBM: the resident overflow index against a numpy cumsum; the three store entries
against the per-recording CPU checkers (tests/ncaltech_ref.py, ncaltech_ts_ref.py, agg_ts_ref.py, each pinned to a fixture recorded from the
reference) and, bit for bit, against the packed entries on the same recordings; independence of the rest of the store; indices that name
no recording; unaligned buffers; ``NCaltechStore`` and its loaders, eagerly and replayed from a captured graph; the experiment's
``train_input = 'atis_store'`` and a short Trainer run.  Counts are integers and both surfaces are bit-reproducible, so the store entries
are compared for equality with the packed ones; against the float64 checkers the surfaces take the comparison of test_gpu_ncaltech_ts.py
(count * 2^-47 per bin) and test_gpu_agg_timesurface.py (rtol 1e-13 and the exact integer exponent)."""
import types

import numpy as np
import pytest
import torch

import agg_ts_ref
import labels_ref
import ncaltech_ref
import ncaltech_ts_ref
from eas_snn_amd import _lib, data, ops

pytestmark = pytest.mark.gpu

H, W, TM = 12, 16, 3
CANVAS = (24, 24)
NEGATIVE = (-20_000, 0)
CONFIGS = [(1, None), (2, None), (1, NEGATIVE), (2, NEGATIVE)]
TS_TAU, SURFACE_TAU = 500e3, 10e3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


def recording(seed, n_events, lead=0, trail=0, t_lo=0, span=60_000):
    """the byte image of a recording: ``n_events`` events over ``span`` us from ``t_lo`` (a few of them outside the 12 x 16 sensor), an
    overflow record in front of the first event of every further 8192 us, ``lead`` more in front of everything (``t_lo`` makes room for
    them) and ``trail`` behind the last event"""
    rng = np.random.default_rng(seed)
    t_lo = max(t_lo, lead * data.ATIS_TIME_INCREMENT)
    t = np.sort(rng.integers(t_lo, t_lo + span, size=n_events, dtype=np.int64))
    x, y, p = rng.integers(0, W + 1, n_events), rng.integers(0, H + 1, n_events), rng.integers(0, 2, n_events)
    marks = np.arange(lead + 1, (t_lo + span) // data.ATIS_TIME_INCREMENT + 1) * data.ATIS_TIME_INCREMENT
    before = np.concatenate([np.zeros(lead, np.int64), np.searchsorted(t, marks), np.full(trail, n_events, np.int64)])
    return data.encode_atis(t, x, y, p, overflow_before=before)


def sized(seed, n_records, **kw):
    """``recording`` with exactly ``n_records`` records: events are taken away until the overflow records fit"""
    n = n_records
    while True:
        buf = recording(seed, n, **kw)
        if len(buf) // 5 == n_records:
            return buf
        n -= len(buf) // 5 - n_records
        assert n > 0


@pytest.fixture(scope='module')
def bufs():
    """the store, in buffer order.  0: the first of the buffer; 1: empty; 2: one event; 3 .. 5: 255, 256, 257 records; 6: ends in four
    overflow records, which share a chunk with the first records of 7; 8: overflow records only; 9: begins with three overflow records;
    10: the last of the buffer, 3000 records"""
    out = [sized(1, 700), np.zeros(0, np.uint8), sized(2, 1, span=8000), sized(3, 255), sized(4, 256), sized(5, 257),
           recording(6, 120, trail=4), recording(7, 300), recording(8, 0, trail=5), recording(9, 150, lead=3), sized(10, 3000)]
    assert [len(b) // 5 for b in out[:6]] == [700, 0, 1, 255, 256, 257] and len(out[10]) // 5 == 3000
    assert (out[8].reshape(-1, 5)[:, 1] == 240).all() and (out[9].reshape(-1, 5)[:3, 1] == 240).all() and out[9].reshape(-1, 5)[3, 1] != 240
    assert (out[6].reshape(-1, 5)[-4:, 1] == 240).all()
    start7 = sum(len(b) // 5 for b in out[:7])
    assert start7 % 256 >= 4                                                    # 6's trailing overflow records lie in 7's first chunk
    return out


BATCH = [10, 3, 0, 7, 1, 5, 8, 2, 9, 4, 6, 7]              # a permutation of the store, 7 twice


def on_device(dev, bufs, shift=0):
    """the recordings back to back, ``shift`` bytes behind an aligned address -> (records, file_offsets, index) on the device"""
    buf = np.concatenate(bufs)
    off = np.cumsum([0] + [len(b) // 5 for b in bufs]).astype(np.int64)
    space = torch.zeros(len(buf) + 8, dtype=torch.uint8, device=dev)
    assert space.data_ptr() % 16 == 0
    rec = space[shift:shift + len(buf)]
    rec.copy_(torch.from_numpy(buf))
    return rec, torch.from_numpy(off).to(dev), ops.atis_store_index(rec)


STORE_OPS = {'count': (ops.event_histogram_atis_store, ops.event_histogram_atis, {}),
             'timesurface': (ops.event_timesurface_atis_store, ops.event_timesurface_atis, {'tau': TS_TAU}),
             'latest': (ops.event_latest_surface_atis_store, ops.event_latest_surface_atis, {'tau': SURFACE_TAU})}


def run_store(kind, held, batch, Tl, window, max_file_records=3000):
    rec, off, index = held
    idx = torch.tensor(batch, dtype=torch.int64, device=rec.device)
    frames, oob, flags = STORE_OPS[kind][0](rec, off, index, idx, Tl, TM, H, W, window=window, return_oob=True, return_flags=True,
                                            max_file_records=max_file_records, **STORE_OPS[kind][2])
    assert frames.shape == (len(batch), Tl, TM, 2, H, W) and frames.dtype == (torch.int32 if kind == 'count' else torch.float64)
    assert oob.shape == flags.shape == (len(batch),)
    return frames, oob, flags


_WANT = {}


def want_of(bufs, i, Tl, window):
    """the checkers' answers for recording ``i``, computed once: dict(count, ts, latest) of (frames, oob, flags)"""
    key = (i, Tl, window)
    if key not in _WANT:
        count = ncaltech_ref.atis_frames(bufs[i], window, Tl, TM, H, W)
        ts = ncaltech_ts_ref.atis_timesurface_frames(bufs[i], window, Tl, TM, H, W, tau=TS_TAU)
        latest = agg_ts_ref.atis_latest_surface(bufs[i], window, Tl, TM, H, W, tau=SURFACE_TAU)
        _WANT[key] = dict(count=count, ts=(ts[0], ts[2], ts[3]), latest=latest)
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ the index
@pytest.mark.parametrize('nrec', [0, 1, 255, 256, 257, 1100 * 256 + 3])
def test_index_is_the_exclusive_cumsum_of_the_chunk_counts(dev, nrec):
    rng = np.random.default_rng(nrec)
    rec = rng.integers(0, 256, size=(nrec, 5), dtype=np.uint8)
    rec[rng.random(nrec) < 0.2, 1] = 240
    chunks = (nrec + 255) // 256
    per = np.add.reduceat((rec[:, 1] == 240).astype(np.int64), np.arange(0, nrec, 256)) if nrec else np.zeros(0, np.int64)
    want = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    index = ops.atis_store_index(torch.from_numpy(rec.reshape(-1)).to(dev))
    assert index.dtype == torch.int32 and index.shape == (chunks + 1,) and len(want) == chunks + 1
    assert np.array_equal(index.cpu().numpy().view(np.uint32), want)
    assert nrec < 1000 or (want[-1] > 50_000 and chunks > 1024)                 # the long case crosses the scan's segments


# ------------------------------------------------------------------------------------------------ the entries
@pytest.mark.parametrize('Tl,window', CONFIGS)
def test_store_entries_equal_the_per_recording_checkers(dev, bufs, Tl, window):
    held = on_device(dev, bufs)
    counts, oob, flags = (v.cpu().numpy() for v in run_store('count', held, BATCH, Tl, window))
    ts, ts_oob, ts_flags = (v.cpu().numpy() for v in run_store('timesurface', held, BATCH, Tl, window))
    lat, lat_oob, lat_flags = (v.cpu().numpy() for v in run_store('latest', held, BATCH, Tl, window))
    binned = 0
    for b, i in enumerate(BATCH):
        want = want_of(bufs, i, Tl, window)
        what = f'recording {i} at {b}, Tl {Tl}, window {window}'
        assert np.array_equal(counts[b], want['count'][0]) and oob[b] == want['count'][1] and flags[b] == want['count'][2], what
        binned += int(counts[b].sum())
        n, err = counts[b], np.abs(ts[b] - want['ts'][0])
        assert (err <= n * 2.0 ** -47).all() and not ts[b][n == 0].any() and (ts[b][n > 0] > 0).all(), what
        assert ts_oob[b] == want['ts'][1] and ts_flags[b] == want['ts'][2], what
        assert lat_oob[b] == want['latest'][1] and lat_flags[b] == want['latest'][2], what
        for k in range(Tl):
            w = want['latest'][0][k]
            if not w.any():                                                     # an empty macro slice, or one of micro window 0
                assert not lat[b, k].any(), what
                continue
            np.testing.assert_allclose(lat[b, k], w, rtol=1e-13, atol=0, err_msg=what)
            assert np.array_equal(agg_ts_ref.exponent_ticks(lat[b, k], SURFACE_TAU), agg_ts_ref.exponent_ticks(w, SURFACE_TAU)), what
    assert binned > 1000 and oob.sum() > 100
    # the empty recording, the one of overflow records only and the single event bin nothing; the repeated index gives the same rows twice
    assert not counts[[4, 6, 7]].any() and (flags[[4, 6, 7]] & 2).all() and not (flags & 16).any()
    assert np.array_equal(counts[3], counts[11]) and np.array_equal(ts[3], ts[11]) and np.array_equal(lat[3], lat[11]) and counts[3].any()


@pytest.mark.parametrize('Tl,window', CONFIGS)
def test_store_entries_equal_the_packed_entries_bit_for_bit(dev, bufs, Tl, window):
    held = on_device(dev, bufs)
    packed, packed_off, _ = on_device(dev, [bufs[i] for i in BATCH])
    for kind, (_, packed_op, tau) in STORE_OPS.items():
        frames, oob, flags = run_store(kind, held, BATCH, Tl, window)
        want = packed_op(packed, packed_off, Tl, TM, H, W, window=window, return_oob=True, return_flags=True, **tau)
        assert torch.equal(frames, want[0]) and torch.equal(oob, want[1]) and torch.equal(flags, want[2]), kind
        assert frames.any() and not (flags & ~15).any()
        # the grid is sized by max_file_records: any bound gives the same frames
        for bound in (0, 255, 1 << 30):
            assert torch.equal(run_store(kind, held, BATCH, Tl, window, max_file_records=bound)[0], frames), (kind, bound)


def test_frames_do_not_depend_on_the_rest_of_the_store(dev, bufs):
    """a recording of an odd record count with overflow records in front of the store and another behind it: every chunk boundary and every
    prefix moves, no frame does"""
    front, back = recording(31, 71, lead=2, trail=1), recording(32, 44, trail=3)
    assert (len(front) // 5) % 2 == 1 and (len(front) // 5) % 256 != 0
    held, moved = on_device(dev, bufs), on_device(dev, [front] + bufs + [back])
    for kind in STORE_OPS:
        a = run_store(kind, held, BATCH, 2, NEGATIVE)
        b = run_store(kind, moved, [i + 1 for i in BATCH], 2, NEGATIVE)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), kind
        assert a[0].any()


def test_indices_outside_the_store_give_zero_frames_and_flag_16(dev, bufs):
    held = on_device(dev, bufs)
    F = len(bufs)
    for kind in STORE_OPS:
        frames, oob, flags = run_store(kind, held, [-1, 3, F, 10, 1 << 40, -(1 << 40)], 2, None)
        good = run_store(kind, held, [3, 10], 2, None)
        assert not frames[[0, 2, 4, 5]].any() and flags[[0, 2, 4, 5]].tolist() == [18] * 4 and not oob[[0, 2, 4, 5]].any(), kind
        assert torch.equal(frames[[1, 3]], good[0]) and torch.equal(oob[[1, 3]], good[1]) and torch.equal(flags[[1, 3]], good[2]), kind
        assert frames[1].any() and frames[3].any() and not (flags[[1, 3]] & 16).any()


@pytest.mark.parametrize('shift', [1, 2, 3])
def test_a_buffer_at_any_alignment_gives_the_same_frames(dev, bufs, shift):
    held, shifted = on_device(dev, bufs), on_device(dev, bufs, shift)
    assert shifted[0].data_ptr() % 4 == shift and torch.equal(held[2], shifted[2])
    for kind in STORE_OPS:
        a, b = run_store(kind, held, BATCH, 2, NEGATIVE), run_store(kind, shifted, BATCH, 2, NEGATIVE)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), kind


# ------------------------------------------------------------------------------------------------ the store and its loaders
def annotated(bufs):
    """the recordings as ``NCaltechStore`` takes them: three classes; boxes inside the sensor, across its border, with a negative corner"""
    boxes = [(2, 1, 11, 9), (9, 6, 20, 15), (-3, -2, 8, 7), (4, 3, 5, 11)]
    return [(f'class_{i % 3}', f'image_{i:04d}', b, data.encode_ncaltech_annotation(*boxes[i % 4])) for i, b in enumerate(bufs)]


def exp_for(kind, Tl=2):
    e = types.SimpleNamespace(Tm=TM, Tl=Tl, input_size=CANVAS, test_size=CANVAS, num_classes=3, window=-20)
    if kind == 'timesurface':
        e.measure = 'timesurface'
    if kind == 'latest':
        e.aggregation, e.measure = 'timesurface', 'timesurface'                 # the aggregation decides, as in atis_to_frames
    return e


@pytest.fixture(scope='module')
def store(dev, bufs):
    return data.NCaltechStore(annotated(bufs), 2, NEGATIVE, dev, sensor_hw=(H, W))


def chain_by_hand(store, kind, idx, par, canvas=CANVAS):
    """the store entry, then the cubic letterbox of its dtype"""
    frames = STORE_OPS[kind][0](store.records, store.file_offsets, store.index, idx, store.Tl, TM, H, W, window=store.window,
                                max_file_records=store.max_file_records, **STORE_OPS[kind][2])
    op = ops.counts_letterbox if kind == 'count' else ops.frames_letterbox
    return op(frames, par, canvas[0], canvas[1], interp='cubic')


PARAMS = [(24, 18, 0, 0, 0), (20, 14, 3, 1, 1), (16, 12, 5, 3, 0), (21, 16, 2, 3, 1)]


@pytest.mark.parametrize('kind', ['count', 'timesurface', 'latest'])
def test_store_frames_and_targets_equal_the_chain_by_hand(dev, store, kind):
    assert len(store) == 11 and store.records.is_cuda and store.index.is_cuda and store.max_file_records == 3000
    assert store.sample_names[4] == 'class_1-image_0004' and store.class_names == ['class_0', 'class_1', 'class_2']
    ids = [10, 0, 7, 1, 9, 7]
    par = np.array([PARAMS[b % 4] for b in range(len(ids))], dtype=np.int32)
    idx, par_dev = torch.tensor(ids, device=dev), torch.from_numpy(par).to(dev)
    got = store.frames(idx, par_dev, exp_for(kind))
    assert got.shape == (6, 2, TM, 2, *CANVAS) and got.dtype == torch.float32 and got.any()
    assert torch.equal(got, chain_by_hand(store, kind, idx, par_dev))
    assert torch.equal(store.frames(idx, par, exp_for(kind)), got)              # params as anything numpy reads
    assert not got[3].any()                                                     # the empty recording
    other = store.frames(idx, par_dev, exp_for(kind), canvas_hw=(20, 28))
    assert other.shape == (6, 2, TM, 2, 20, 28)
    targets, count, flags = store.targets(idx, par_dev, CANVAS, return_info=True)
    want = labels_ref.targets(store.host['boxes'], store.host['group_start'], ids, par, H, W, *CANVAS)
    assert np.array_equal(targets.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1]) and not flags.any()
    assert count.sum() >= 3 and targets.shape == (6, 50, 5)
    with pytest.raises(ValueError):
        store.frames(idx, par_dev, types.SimpleNamespace(Tm=TM, input_size=CANVAS, measure='voxel'))


def test_training_loader_first_batch_equals_the_chain(dev, store):
    exp = exp_for('count')
    loader = data.NCaltechStoreLoader(exp, 4, store=store, seed=2)
    assert len(loader) == 2 and len(loader.dataset) == 11
    idx, par = loader.batches(0)[0]
    frames, targets = next(iter(loader))
    assert frames.shape == (4, 2, TM, 2, *CANVAS) and frames.device == dev and targets.shape == (4, 50, 5) and targets.device == dev
    assert torch.equal(frames, chain_by_hand(store, 'count', torch.from_numpy(idx).to(dev), torch.from_numpy(par).to(dev)))
    assert np.array_equal(targets.cpu().numpy(), labels_ref.targets(store.host['boxes'], store.host['group_start'], idx, par, H, W, *CANVAS)[0])
    assert loader.epoch == 1 and frames.any()


def test_eval_loader_yields_the_evaluation_tuple(dev, store):
    exp = exp_for('count')
    loader = data.NCaltechStoreEvalLoader(exp, 4, [0, 5, 9, 2, 10, 7], store)
    assert len(loader) == 2 and loader.dataset.sample_names is store.sample_names and loader.dataset.map_val and not loader.dataset.random_aug
    assert loader.dataset.class_names == store.class_names and len(loader.dataset) == 11
    row = data.letterbox_params(H, W, *CANVAS)
    assert row == (24, 18, 0, 0, 0)
    for (frames, labels, (hs, ws), ids), want_ids in zip(loader, ([0, 5, 9, 2], [10, 7])):
        assert ids.tolist() == want_ids and hs.tolist() == [H] * len(want_ids) and ws.tolist() == [W] * len(want_ids)
        par = torch.tensor([row] * len(want_ids), dtype=torch.int32, device=dev)
        assert torch.equal(frames, chain_by_hand(store, 'count', torch.tensor(want_ids, device=dev), par)) and frames.shape[0] == len(want_ids)
        for i, lab in zip(want_ids, labels):
            assert lab.dtype == torch.float32 and not lab.is_cuda and lab.shape == (1, 5) and np.array_equal(lab.numpy(), store.raw_labels(i))
            assert store.sample_names[i] == f'class_{i % 3}-image_{i:04d}' and lab[0, 4] == i % 3


def test_frames_and_targets_replay_from_a_captured_graph(dev, store):
    exp = exp_for('timesurface')
    loader = data.NCaltechStoreLoader(exp, 4, store=store, seed=5)
    (i0, p0), (i1, p1) = loader.batches(0)[:2]
    idx, par = torch.from_numpy(i0).to(dev), torch.from_numpy(p0).to(dev)

    def chain():
        return store.frames(idx, par, exp), store.targets(idx, par, exp.input_size)
    side = _lib.private_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                             # allocator warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            frames, targets = chain()                                       # no host read inside: the capture would fail
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    eager_frames, eager_targets = chain()
    assert torch.equal(frames, eager_frames) and torch.equal(targets, eager_targets) and frames.any()
    # new indices and draws in the captured tensors: the replay follows them
    idx.copy_(torch.from_numpy(i1))
    par.copy_(torch.from_numpy(p1))
    frames.zero_()
    targets.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    eager_frames, eager_targets = chain()
    assert torch.equal(frames, eager_frames) and torch.equal(targets, eager_targets)
    assert np.array_equal(targets.cpu().numpy(), labels_ref.targets(store.host['boxes'], store.host['group_start'], i1, p1, H, W, *CANVAS)[0])
    assert not np.array_equal(i0, i1)


# ------------------------------------------------------------------------------------------------ the experiment
def test_experiment_hands_out_the_store_loaders_when_asked(dev):
    from yolox.exp import get_exp
    e = get_exp(None, 'e-yolox-s')
    e.train_input, e.atis_store_recordings = 'atis_store', (8, 3000)
    e.merge(['input_size', '(64, 64)', 'test_size', '(64, 64)', 'num_classes', '2'])
    loader = e.get_data_loader(4, False)
    assert isinstance(loader, data.NCaltechStoreLoader) and len(loader) == 2 and loader.store.sensor_hw == (64, 64)
    assert e.get_data_loader(4, False).store is loader.store                    # one store per split, kept on the experiment
    assert isinstance(e.get_eval_dataset(), data.NCaltechStoreDataset)
    ev = e.get_eval_loader(2, False)
    assert isinstance(ev, data.NCaltechStoreEvalLoader) and ev.batch_size == 4 and ev.store is not loader.store and len(ev.dataset) == 8
    assert loader.store.class_names == ['class_000', 'class_001'] and loader.store.Tl == e.Tl


def test_trainer_loop_on_the_store_loader(dev, tmp_path, monkeypatch):
    """two iterations of ``yolox.core.Trainer.train()`` (default Adam) fed by ``train_input = 'atis_store'`` at 64 x 64: the step is
    recorded and replayed as with the synthetic loader, and it trains"""
    from yolox.exp import get_exp
    monkeypatch.setattr(ops, 'VERIFY_SMALL_INT', False)      # the suite's tag check reads the device: not inside a capture
    exp = get_exp(None, 'e-yolox-s')
    exp.merge(['T', '3', 'embedding', 'arsnn', 'num_classes', '2', 'spike_attach', 'True', 'thresh', '1', 'readout', 'sum', 'embedding_depth', '2',
               'embedding_ksize', '5', 'write_zero', 'True', 'spike_fn', 'atan'] + ['use_spike', 'True', 'input_size', '(64, 64)', 'test_size', '(64, 64)'])
    exp.max_epoch, exp.print_interval, exp.output_dir = 1, 1, str(tmp_path)
    exp.train_input, exp.atis_store_recordings = 'atis_store', (8, 3000)
    torch.manual_seed(5)
    tr = exp.get_trainer(types.SimpleNamespace(batch_size=4, fp16=False, experiment_name='atis_store', ckpt=None, resume=False))
    tr.train()
    assert isinstance(tr.train_loader, data.NCaltechStoreLoader) and len(tr.train_loader) == 2
    assert len(tr.log) == 2 and all(np.isfinite(r['loss']) for r in tr.log)
    torch.cuda.set_stream(torch.cuda.default_stream())
