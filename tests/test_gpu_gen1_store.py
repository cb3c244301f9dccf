"""GPU tests of Gen1 training from recordings in HBM: ``ops.label_targets`` against the fixture recorded from the reference
(tests/golden/gen1_labels.npz) and against the numpy checker (tests/labels_ref.py, pinned to that fixture by test_cpu_gen1_store.py) at the
shapes where the kernel can go wrong; ``Gen1Store.frames`` against the chain on ranges searched by hand; the loaders, eagerly and replayed
from a captured graph; the experiment's ``train_input = 'dat_store'`` and a short Trainer run.  Every value is an integer or a half below
2^24 and the only rounding is one IEEE double division, so every comparison is exact."""
import types
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

import labels_ref
from eas_snn_amd import _lib, data, ops

pytestmark = pytest.mark.gpu

SENSOR, CANVAS = (240, 304), (256, 320)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


def run(dev, boxes, group_start, group, params, sensor, canvas, perm=None, max_labels=50):
    """the op and the checker on the same numpy inputs; asserts that they agree and returns the op's (targets, count, flags)"""
    t, count, flags = ops.label_targets(torch.from_numpy(np.asarray(boxes, dtype=np.float32).reshape(-1, 5)).to(dev),
                                        torch.tensor(list(group_start), dtype=torch.int64, device=dev),
                                        torch.tensor(list(group), dtype=torch.int64, device=dev),
                                        torch.tensor(np.asarray(params).reshape(-1, 5), dtype=torch.int32, device=dev), *sensor, *canvas,
                                        perm=None if perm is None else torch.tensor(np.asarray(perm), dtype=torch.int32, device=dev),
                                        max_labels=max_labels, return_info=True)
    B = len(group)
    assert t.shape == (B, max_labels, 5) and t.dtype == torch.float32 and count.shape == flags.shape == (B,) and count.dtype == flags.dtype == torch.int32
    t, count, flags = t.cpu().numpy(), count.cpu().numpy(), flags.cpu().numpy()
    want = labels_ref.targets(boxes, group_start, group, params, *sensor, *canvas, perm=perm, max_labels=max_labels)
    assert np.array_equal(t, want[0]) and np.array_equal(count, want[1]) and np.array_equal(flags, want[2])
    return t, count, flags


def test_label_targets_equals_the_reference_fixture(dev):
    """every case of a geometry as one batch: the box table is the cases' rows back to back, a group per case, the recorded permutations"""
    cases = list(labels_ref.fixture_cases(load_golden('gen1_labels')))
    for geo in ('gen1', 'small'):
        mine = [c for n, c in cases if n.startswith(geo + '_')]
        assert len(mine) == 24
        sensor, canvas = mine[0]['sensor'], mine[0]['canvas']
        boxes = np.concatenate([c['raw'] for c in mine])
        group_start = np.cumsum([0] + [len(c['raw']) for c in mine])
        params = [labels_ref.case_params(c) for c in mine]
        perm = np.tile(np.arange(70), (len(mine), 1))
        for b, c in enumerate(mine):
            perm[b, :len(c['perm'])] = c['perm']
        t, count, flags = run(dev, boxes, group_start, range(len(mine)), params, sensor, canvas, perm=perm)
        assert np.array_equal(t, np.stack([c['targets'] for c in mine])) and list(count) == [len(c['rows']) for c in mine] and not flags.any()
        assert count.max() == 70 and count.min() == 0


def random_boxes(rng, n, drop_every=0):
    """n rows on the Gen1 sensor, some with negative corners; every ``drop_every``-th one is a box without area"""
    x, y = rng.uniform(-20, 250, n), rng.uniform(-15, 190, n)
    box = np.stack([x, y, x + rng.uniform(8, 120, n), y + rng.uniform(8, 100, n), rng.integers(0, 3, n)], axis=-1)
    if drop_every:
        box[::drop_every, 2:4] = box[::drop_every, 0:2]
    return box.astype(np.float32)


@pytest.mark.parametrize('order', ['none', 'identity', 'reversed', 'random'])
def test_label_targets_group_sizes_around_the_wave_chunk(dev, order):
    """groups of 0, 1, 63, 64, 65 and 70 rows (a wave walks 64 rows at a time), every third row without area, flip off and on, both cuts"""
    rng = np.random.default_rng(11)
    sizes = [0, 1, 63, 64, 65, 70]
    boxes = np.concatenate([random_boxes(rng, n, drop_every=3) for n in sizes])
    group_start = np.cumsum([0] + sizes)
    group = list(range(6)) * 2
    params = [(250, 200, 30, 20, 0)] * 6 + [(199, 231, 77, 9, 1)] * 6
    perm = None
    if order != 'none':
        perm = np.tile(np.arange(70), (12, 1))
        for b, g in enumerate(group):
            n = sizes[g]
            perm[b, :n] = {'identity': np.arange(n), 'reversed': np.arange(n)[::-1], 'random': rng.permutation(n)}[order]
    for max_labels in (50, 1):
        t, count, flags = run(dev, boxes, group_start, group, params, SENSOR, CANVAS, perm=perm, max_labels=max_labels)
        assert not flags.any() and count[0] == 0 and count[5] > 40 and not t[0].any()
    # the order of the rows is the order of the targets: the permuted op equals the identity op on the table permuted by hand
    if order in ('reversed', 'random'):
        moved = np.concatenate([boxes[group_start[g]:group_start[g + 1]][perm[g, :sizes[g]]] for g in range(6)])
        same, _, _ = run(dev, moved, group_start, group[:6], params[:6], SENSOR, CANVAS)
        assert np.array_equal(same, t_at(dev, boxes, group_start, group[:6], params[:6], perm[:6]))


def t_at(dev, boxes, group_start, group, params, perm):
    return run(dev, boxes, group_start, group, params, SENSOR, CANVAS, perm=perm)[0]


def test_label_targets_cut_at_fifty_on_either_side_of_row_64(dev):
    """70 rows that survive unless made empty: the 50th survivor is row 49 (first chunk of the wave) or row 68 (second chunk), and the
    rows behind it are cut"""
    rng = np.random.default_rng(12)
    x, y = rng.uniform(20, 150, 70), rng.uniform(20, 100, 70)
    full = np.stack([x, y, x + rng.uniform(30, 100, 70), y + rng.uniform(30, 90, 70), np.arange(70) % 3], axis=-1).astype(np.float32)
    late = full.copy()
    late[:19, 2:4] = late[:19, 0:2]                                            # rows 0 .. 18 leave: survivor 50 is row 68, survivor 51 row 69
    boxes, group_start = np.concatenate([full, late]), [0, 70, 140]
    params = [(280, 230, 10, 5, 0), (280, 230, 10, 5, 1)]
    for group in ([0, 1], [1, 0]):
        t, count, flags = run(dev, boxes, group_start, group, params, SENSOR, CANVAS)
        assert sorted(count) == [51, 70] and not flags.any() and t[:, 49].any(axis=-1).all()
    one = labels_ref.sample_targets(late[68:69], params[0], *SENSOR, *CANVAS)[0]
    t, _, _ = run(dev, boxes, group_start, [1], params[:1], SENSOR, CANVAS)
    assert np.array_equal(t[0, 49], one[0])                                    # row 68 sits in the last kept slot
    # a reversed list moves the cut to the other end
    t, count, _ = run(dev, boxes, group_start, [1], params[:1], SENSOR, CANVAS, perm=np.arange(70)[None, ::-1].copy())
    assert count[0] == 51 and np.array_equal(t[0, 0], labels_ref.sample_targets(late[69:70], params[0], *SENSOR, *CANVAS)[0][0])


def test_label_targets_flags_counts_and_the_empty_batch(dev):
    rng = np.random.default_rng(13)
    sizes = [0, 70, 5]
    boxes = np.concatenate([random_boxes(rng, n) for n in sizes])
    group_start = np.cumsum([0] + sizes)
    group = [0, 1, 3, -1, 2, 2, 1]
    params = [(304, 240, 0, 0, 0)] * 4 + [(150, 100, 60, 70, 1)] * 3
    perm = np.tile(np.arange(8), (7, 1))
    perm[4, :5] = [4, 9, 0, -1, 2]                                             # two entries outside the group of 5 rows
    perm[5, :5] = [3, 1, 4, 0, 2]
    t, count, flags = run(dev, boxes, group_start, group, params, SENSOR, CANVAS, perm=perm)
    assert list(flags) == [0, 2, 4, 4, 1, 0, 2] and count[0] == count[2] == count[3] == 0 and count[1] <= 8 and count[4] <= 3 and count[6] <= 8
    assert not t[0].any() and not t[2].any() and not t[3].any()
    t1, count1, flags1 = run(dev, boxes, group_start, group, params, SENSOR, CANVAS, perm=perm, max_labels=1)
    assert np.array_equal(t1, t[:, :1]) and np.array_equal(count1, count) and np.array_equal(flags1, flags)
    # B = 0: nothing to do, shapes kept
    z = torch.zeros
    t0, c0, f0 = ops.label_targets(torch.from_numpy(boxes).to(dev), torch.tensor(group_start, device=dev), z(0, dtype=torch.int64, device=dev),
                                   z(0, 5, dtype=torch.int32, device=dev), *SENSOR, *CANVAS, return_info=True)
    assert t0.shape == (0, 50, 5) and c0.shape == (0,) and f0.shape == (0,)
    only = ops.label_targets(torch.from_numpy(boxes).to(dev), torch.tensor(group_start, device=dev), torch.tensor([1], device=dev),
                             torch.tensor([params[0]], dtype=torch.int32, device=dev), *SENSOR, *CANVAS)
    assert torch.is_tensor(only) and only.shape == (1, 50, 5)


# ------------------------------------------------------------------------------------------------ the store
def gap_recordings():
    """two recordings on a 24 x 32 sensor; the first has no event between 1.1 s and 1.3 s, and a label inside that gap"""
    rng = np.random.default_rng(21)
    out = []
    for f, spans in enumerate((((1_000_000, 1_100_000), (1_300_000, 1_400_000)), ((2_000_000, 2_300_000),))):
        t = np.sort(np.concatenate([rng.integers(a, b, 1500) for a, b in spans]))
        x, y, p = rng.integers(0, 32, len(t)), rng.integers(0, 24, len(t)), rng.integers(0, 2, len(t))
        times = (1_050_000, 1_250_000, 1_350_000) if f == 0 else (2_040_000, 2_150_000)
        rows = [(lt, 4 + k, 3, 12, 9 + k, k % 2, 1.0, 0) for k, lt in enumerate(times)] + [(times[-1], 10, 8, 15, 12, 1, 1.0, 1)]
        out.append((f'rec{f}', data.encode_dat(t, x, y, p, 24, 32), np.array(rows, dtype=data.GEN1_BBOX_DTYPE)))
    return out


def chain_by_hand(store, ids, params, Tm, canvas, aggregation='micro_sum'):
    """frames of the samples ``ids``: one window search per sample and macro slice, then the chain on the collected ranges"""
    dev, step = store.records.device, store.window[1] - store.window[0]
    ranges, rows = [], []
    for i, par in zip(ids, params):
        for k in range(-store.Tl + 1, 1):
            t = torch.tensor([int(store.host['group_t'][i]) + k * step], dtype=torch.int64, device=dev)
            f = torch.tensor([int(store.host['group_file'][i])], dtype=torch.int32, device=dev)
            ranges.append(ops.event_window_search(store.records, t, store.window, store.Tl, store.file_offsets, f))
            rows.append(par)
    out = data.dat_ranges_to_frames(store.records, torch.cat(ranges), Tm, store.sensor_hw, canvas, rows, aggregation=aggregation)
    return out.reshape(len(ids), store.Tl, Tm, 2, *canvas), torch.cat(ranges).cpu().numpy()


@pytest.mark.parametrize('Tl', [1, 2])
def test_store_frames_equal_the_chain_on_ranges_searched_by_hand(dev, Tl):
    exp = types.SimpleNamespace(Tm=3, Tl=Tl, input_size=(32, 48))
    store = data.Gen1Store(gap_recordings(), Tl, (-20_000, 0), dev, sensor_hw=(24, 32))
    assert len(store) == 5 and store.records.is_cuda and store.group_start.tolist() == [0, 1, 2, 4, 5, 7]
    ids = [4, 1, 0, 2, 3]
    params = [(32, 24, 0, 0, 0), (40, 30, 3, 1, 1), (20, 15, 9, 11, 0), (32, 24, 16, 8, 1), (25, 22, 2, 3, 0)]
    idx = torch.tensor(ids, device=dev)
    par = torch.tensor(params, dtype=torch.int32, device=dev)
    want, ranges = chain_by_hand(store, ids, params, 3, (32, 48))
    got = store.frames(idx, par, exp)
    assert got.shape == (5, Tl, 3, 2, 32, 48) and got.dtype == torch.float32 and torch.equal(got, want)
    ranges = ranges.reshape(5, Tl, 2)
    assert (ranges[1, :, 0] == ranges[1, :, 1]).all() and not got[1].any()     # the label in the gap: empty windows, zero frames
    assert all(got[b].any() for b in (0, 2, 3, 4)) and (ranges[[0, 2, 3, 4], -1, 1] > ranges[[0, 2, 3, 4], -1, 0]).all()
    assert (ranges[0] >= 3000).all() and (ranges[[1, 2, 3]] <= 3000).all()      # every range stays inside its recording
    exp.aggregation = 'timesurface'
    assert torch.equal(store.frames(idx, par, exp), chain_by_hand(store, ids, params, 3, (32, 48), 'timesurface')[0])


def small_exp():
    return types.SimpleNamespace(Tm=3, Tl=1, input_size=(32, 48), test_size=(32, 48), num_classes=2, window=-20)


@pytest.fixture(scope='module')
def small_store(dev):
    return data.Gen1Store(data.synth_gen1_recordings(2, 8, n_events=3000, sensor_hw=(24, 32), seed=6), 1, (-20_000, 0), dev, sensor_hw=(24, 32))


def test_loader_frames_and_targets(dev, small_store):
    exp, store = small_exp(), small_store
    loader = data.Gen1StoreLoader(exp, 4, store=store, seed=2)
    assert len(loader) == 4 and len(loader.dataset) == 16
    draws = loader.batches(0)
    n, kept = 0, 0
    for (frames, targets), (idx, par, perm) in zip(loader, draws):
        assert frames.shape == (4, 1, 3, 2, 32, 48) and frames.dtype == torch.float32 and frames.device == dev
        assert targets.shape == (4, 50, 5) and targets.dtype == torch.float32 and targets.device == dev
        assert torch.equal(frames, chain_by_hand(store, idx, [tuple(int(v) for v in p) for p in par], 3, (32, 48))[0]) and frames.any()
        want, count, flags = labels_ref.targets(store.host['boxes'], store.host['group_start'], idx, par, 24, 32, 32, 48, perm=perm)
        assert np.array_equal(targets.cpu().numpy(), want) and not flags.any()
        kept += int(count.sum())
        n += 1
    assert n == 4 and loader.epoch == 1 and kept > 8
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(loader.batches(1), draws))


def test_eval_loader_yields_the_evaluation_tuple(dev, small_store):
    exp, store = small_exp(), small_store
    loader = data.Gen1StoreEvalLoader(exp, 4, [0, 5, 9, 2, 15, 7], store)
    assert len(loader) == 2 and loader.dataset.sample_names is store.sample_names and loader.dataset.map_val and not loader.dataset.random_aug
    assert loader.dataset.class_names == ['0', '1'] and len(loader.dataset) == 16
    row = data.letterbox_params(24, 32, 32, 48)
    for (frames, labels, (hs, ws), ids), want_ids in zip(loader, ([0, 5, 9, 2], [15, 7])):
        assert ids.tolist() == want_ids and hs.tolist() == [24] * len(want_ids) and ws.tolist() == [32] * len(want_ids)
        assert torch.equal(frames, chain_by_hand(store, want_ids, [row] * len(want_ids), 3, (32, 48))[0]) and frames.shape[0] == len(want_ids)
        for i, lab in zip(want_ids, labels):
            assert lab.dtype == torch.float32 and not lab.is_cuda and np.array_equal(lab.numpy(), store.raw_labels(i)) and lab.shape[1] == 5


def test_frames_and_targets_replay_from_a_captured_graph(dev, small_store):
    exp, store = small_exp(), small_store
    loader = data.Gen1StoreLoader(exp, 4, store=store, seed=5)
    (i0, p0, q0), (i1, p1, q1) = loader.batches(0)[:2]
    idx, par, perm = torch.from_numpy(i0).to(dev), torch.from_numpy(p0).to(dev), torch.from_numpy(q0).to(dev)

    def chain():
        return store.frames(idx, par, exp), store.targets(idx, par, perm, exp.input_size)
    side = _lib.private_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                                             # allocator warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            frames, targets = chain()                                       # no host read inside: the capture would fail
    torch.cuda.current_stream().wait_stream(side)
    # new indices, draws and permutations in the captured tensors: the replay follows them
    idx.copy_(torch.from_numpy(i1))
    par.copy_(torch.from_numpy(p1))
    perm.copy_(torch.from_numpy(q1))
    frames.zero_()
    targets.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    eager_frames, eager_targets = chain()
    assert torch.equal(frames, eager_frames) and torch.equal(targets, eager_targets)
    assert np.array_equal(targets.cpu().numpy(), labels_ref.targets(store.host['boxes'], store.host['group_start'], i1, p1, 24, 32, 32, 48, perm=q1)[0])
    assert not np.array_equal(i0, i1)


# ------------------------------------------------------------------------------------------------ the experiment
def test_experiment_hands_out_the_store_loaders_when_asked(dev):
    from yolox.evaluators.psee_evaluator import PSEEEvaluator
    from yolox.exp import get_exp
    e = get_exp(None, 'e-yolox-s')
    assert type(e.get_data_loader(4, False)).__name__ == 'SyntheticEventLoader'
    assert type(e.get_eval_loader(2, False)).__name__ == 'SyntheticEvalLoader'
    e = get_exp(None, 'e-yolox-s')
    e.train_input, e.store_recordings = 'dat_store', (2, 8, 3000)
    e.merge(['input_size', '(64, 64)', 'test_size', '(64, 64)', 'num_classes', '2'])
    loader = e.get_data_loader(4, False)
    assert isinstance(loader, data.Gen1StoreLoader) and len(loader) == 4 and loader.store.sensor_hw == (64, 64)
    assert e.get_data_loader(4, False).store is loader.store                    # one store per split, kept on the experiment
    ev = e.get_eval_loader(2, False)
    assert isinstance(ev, data.Gen1StoreEvalLoader) and ev.batch_size == 4 and ev.store is not loader.store and len(ev.dataset) == 16
    e.eval_proph, e.data_name = True, 'gen1'
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        assert isinstance(e.get_evaluator(2, False), PSEEEvaluator)


def test_trainer_loop_on_the_store_loader(dev, tmp_path, monkeypatch):
    """four iterations of ``yolox.core.Trainer.train()`` (default Adam) fed by ``train_input = 'dat_store'`` at 64 x 64: the step is
    recorded and replayed as with the synthetic loader, and it trains"""
    from yolox.exp import get_exp
    monkeypatch.setattr(ops, 'VERIFY_SMALL_INT', False)      # the suite's tag check reads the device: not inside a capture
    exp = get_exp(None, 'e-yolox-s')
    exp.merge(['T', '3', 'embedding', 'arsnn', 'num_classes', '2', 'spike_attach', 'True', 'thresh', '1', 'readout', 'sum', 'embedding_depth', '2',
               'embedding_ksize', '5', 'write_zero', 'True', 'spike_fn', 'atan'] + ['use_spike', 'True', 'input_size', '(64, 64)', 'test_size', '(64, 64)'])
    exp.max_epoch, exp.print_interval, exp.output_dir = 1, 1, str(tmp_path)
    exp.train_input, exp.store_recordings = 'dat_store', (2, 8, 3000)
    torch.manual_seed(5)
    tr = exp.get_trainer(types.SimpleNamespace(batch_size=4, fp16=False, experiment_name='store', ckpt=None, resume=False))
    tr.train()
    assert isinstance(tr.train_loader, data.Gen1StoreLoader) and len(tr.train_loader) == 4
    assert tr.use_graph and tr.step.graphs is not None
    assert len(tr.log) == 4 and all(np.isfinite(r['loss']) for r in tr.log)
    torch.cuda.set_stream(torch.cuda.default_stream())
