"""GPU tests of store training on N ranks.  Replica mode: the batches of the rank loaders, interleaved, are the single-process loader's
batch, frames and targets.  Shard mode: a rank's store gives, for every sample it owns, the frames and targets of the unsharded store
under the same global index, and holds its share of the record bytes; the ranks' evaluation loaders partition the samples; a short
Trainer run over a sharded store.  Every frame and target here is a count, a half or one IEEE division: every comparison is exact."""
import types

import numpy as np
import pytest
import torch

from eas_snn_amd import data, ops

pytestmark = pytest.mark.gpu

SENSOR, CANVAS = (24, 32), (32, 64)
KINDS = ('gen1', 'window', 'gen4', 'atis')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


def gen1_recs():
    # recordings of different sizes (500 .. 3000 events), so that the weights of the greedy assignment differ
    return [data.synth_gen1_recordings(f + 1, 6, n_events=500 + 1250 * f, sensor_hw=SENSOR, seed=3)[f] for f in range(3)]


def gen4_recs():
    return data.synth_gen4_recordings(3, 12, (12, 16), 10, 3, seed=4)


def atis_recs():
    return data.synth_ncaltech_recordings(12, 3000, sensor_hw=SENSOR, seed=5)


def build(kind, dev, **kw):
    if kind == 'gen1':
        return data.Gen1Store(gen1_recs(), 1, (-20_000, 0), dev, sensor_hw=SENSOR, **kw)
    if kind == 'window':
        return data.Gen1WindowStore(gen1_recs(), 1, (-20_000, 0), dev, sensor_hw=SENSOR, **kw)
    if kind == 'gen4':
        return data.Gen4Store(gen4_recs(), 3, dev, sensor_hw=(12, 16), chunk=5, **kw)
    return data.NCaltechStore(atis_recs(), 1, None, dev, sensor_hw=SENSOR, **kw)


def loader_of(kind):
    return {'gen1': data.Gen1StoreLoader, 'window': data.Gen1StoreLoader, 'gen4': data.Gen4StoreLoader, 'atis': data.NCaltechStoreLoader}[kind]


def kind_exp():
    return types.SimpleNamespace(Tm=3, Tl=1, input_size=CANVAS, test_size=CANVAS, num_classes=3, window=-20)


@pytest.fixture(scope='module')
def whole(dev):
    """the unsharded stores, built once"""
    return {kind: build(kind, dev) for kind in KINDS}


# ------------------------------------------------------------------------------------------------ 6. replica mode
@pytest.mark.parametrize('kind', KINDS)
def test_rank_batches_interleaved_are_the_single_process_batch(dev, whole, kind):
    store, exp, Loader = whole[kind], kind_exp(), loader_of(kind)
    single = Loader(exp, 4, store=store, seed=9)
    ranks = [Loader(exp, 2, store=store, seed=9, rank=r, world=2) for r in range(2)]
    assert len(single) == len(ranks[0]) == len(ranks[1]) == len(store) // 4
    steps = 0
    for (frames, targets), (f0, t0), (f1, t1) in zip(single, *ranks):
        assert frames.shape[0] == 4 and f0.shape == f1.shape == (2,) + frames.shape[1:] and t0.shape == (2, 50, 5)
        assert torch.equal(torch.stack([f0, f1], 1).flatten(0, 1), frames) and frames.any()
        assert torch.equal(torch.stack([t0, t1], 1).flatten(0, 1), targets)
        steps += 1
    assert steps == len(single) and single.epoch == ranks[0].epoch == 1


# ------------------------------------------------------------------------------------------------ 7. shard mode
def fixed_draws(store, exp):
    """params [G, 5] and box permutations [G, P] for every global sample, from one seeded state"""
    rs = np.random.RandomState(17)
    (H, W), (Hc, Wc) = store.sensor_hw, exp.input_size
    G = len(store)
    par = np.array([data.jitter_params(H, W, Hc, Wc, jitter=.3, rng=rs) for _ in range(G)], dtype=np.int32).reshape(G, 5)
    rows = getattr(store, 'group_rows', np.ones(G, dtype=np.int64))
    perm = np.tile(np.arange(max(int(rows.max()), 1), dtype=np.int32), (G, 1))
    for g in range(G):
        perm[g, :rows[g]] = rs.permutation(int(rows[g]))
    return par, perm


def held_bytes(store):
    return store.sums.numel() * 2 if hasattr(store, 'sums') else store.records.numel()


@pytest.mark.parametrize('kind', KINDS)
def test_a_shard_gives_the_frames_and_targets_of_the_unsharded_store(dev, whole, kind):
    full, exp = whole[kind], kind_exp()
    par, perm = fixed_draws(full, exp)
    if kind in ('gen1', 'window'):
        sizes = [len(r[1]) for r in gen1_recs()]                # the weights: the byte images (what a shard reads at build time)
    elif kind == 'gen4':
        sizes = [len(r[1]) * 2 * 12 * 16 * 2 for r in gen4_recs()]      # in bytes of bin sums
    else:
        sizes = [len(r[2]) for r in atis_recs()]
    seen, kept = [], 0
    for r in range(2):
        shard = build(kind, dev, shard=(r, 2))
        assert shard.shard == (r, 2) and shard.sharded and len(shard) == len(full) and shard.sample_names == full.sample_names
        own = shard.owned_samples
        assert 0 < len(own) < len(full)
        idx = torch.from_numpy(own).to(dev)
        p, q = torch.from_numpy(par[own]).to(dev), torch.from_numpy(perm[own]).to(dev)
        got, want = shard.frames(idx, p, exp), full.frames(idx, p, exp)
        assert got.shape[0] == len(own) and torch.equal(got, want) and want.any()
        if kind == 'atis':
            assert torch.equal(shard.targets(idx, p, exp.input_size), full.targets(idx, p, exp.input_size))
        else:
            assert torch.equal(shard.targets(idx, p, q, exp.input_size), full.targets(idx, p, q, exp.input_size))
        assert held_bytes(shard) <= sum(sizes) / 2 + max(sizes)
        if kind == 'window':
            kept += shard.kept_records
            assert shard.sample_ranges.shape == full.sample_ranges.shape and shard.used_bytes == shard.records.numel() == 8 * shard.kept_records
            foreign = torch.from_numpy(np.setdiff1d(np.arange(len(full)), own)).to(dev)
            assert not shard.sample_ranges[foreign].any()                      # the samples of the other rank: empty ranges
        seen += own.tolist()
    assert sorted(seen) == list(range(len(full)))
    if kind == 'window':
        assert kept == full.kept_records
    elif kind != 'gen4':
        assert held_bytes(full) <= sum(sizes)


@pytest.mark.parametrize('kind', KINDS)
def test_shard_loaders_yield_their_own_draws(dev, whole, kind):
    """a step of a loader over a sharded store is the unsharded store's frames and targets at the loader's own draws"""
    full, exp, Loader = whole[kind], kind_exp(), loader_of(kind)
    shard = build(kind, dev, shard=(1, 2))
    loader = Loader(exp, 2, store=shard, seed=4)
    draws = loader.batches(0)
    assert len(draws) == len(loader) >= 1
    for (frames, targets), d in zip(loader, draws):
        idx, p = torch.from_numpy(d[0]).to(dev), torch.from_numpy(d[1]).to(dev)
        assert shard.owns(d[0]).all() and torch.equal(frames, full.frames(idx, p, exp))
        want = full.targets(idx, p, exp.input_size) if kind == 'atis' else full.targets(idx, p, torch.from_numpy(d[2]).to(dev), exp.input_size)
        assert torch.equal(targets, want)


# ------------------------------------------------------------------------------------------------ 8. evaluation over sharded stores
def store_exp(train_input, monkeypatch, rank, world=2):
    import yolox.utils
    from yolox.exp import get_exp
    monkeypatch.setattr(yolox.utils, 'get_rank', lambda: rank)
    monkeypatch.setattr(yolox.utils, 'get_world_size', lambda: world)
    e = get_exp(None, 'e-yolox-s')
    e.train_input = train_input
    e.store_recordings, e.atis_store_recordings = {'hist_store': (3, 12)}.get(train_input, (3, 6, 2000)), (10, 3000)
    e.merge(['input_size', '(32, 32)', 'test_size', '(32, 32)', 'num_classes', '2', 'Tm', '3'])
    return e


def per_id(loader):
    out = {}
    for frames, labels, (hs, ws), ids in loader:
        assert frames.shape[0] == len(labels) == len(hs) == len(ws) == len(ids)
        for k, i in enumerate(ids.tolist()):
            assert i not in out
            out[i] = (frames[k].clone(), labels[k], int(hs[k]), int(ws[k]))
    return out


@pytest.mark.parametrize('train_input', ['dat_store', 'hist_store', 'atis_store'])
def test_sharded_evaluation_sees_every_sample_once_under_its_global_id(dev, monkeypatch, train_input):
    import yolox.utils
    e = store_exp(train_input, monkeypatch, 0)
    want = per_id(e.get_eval_loader(2, False))
    n = len(e.get_eval_dataset())
    assert sorted(want) == list(range(n)) and n >= 10
    e.store_shard = 'recordings'
    got, sizes = {}, []
    for rank in (0, 1):
        monkeypatch.setattr(yolox.utils, 'get_rank', lambda: rank)
        loader = e.get_eval_loader(2, True)
        assert loader.store.shard == (rank, 2) and loader.batch_size == 2 and loader.dataset.sample_names == e.get_eval_dataset().sample_names
        mine = per_id(loader)
        assert sorted(mine) == loader.store.owned_samples.tolist() and not set(mine) & set(got)
        got.update(mine)
        sizes.append(len(mine))
    assert sorted(got) == list(range(n)) and min(sizes) >= 1
    for i in range(n):
        assert torch.equal(got[i][0], want[i][0]) and torch.equal(got[i][1], want[i][1]) and got[i][2:] == want[i][2:]
    assert any(w[0].any() for w in want.values())


# ------------------------------------------------------------------------------------------------ 9. the trainer
def test_trainer_loop_over_a_sharded_store(dev, tmp_path, monkeypatch):
    """``yolox.core.Trainer.train()`` fed by ``train_input = 'dat_store'`` with ``store_shard = 'recordings'`` as rank 0 of a world of 2
    (the launcher's answers are patched, in ``yolox.utils`` and where the trainer has bound them; there is no process group, so the
    gradient exchange stays unbound as on one rank): the rank holds one of the two recordings, the global batch of 8 is 4 per rank, an
    epoch is the rank's 8 samples in 2 steps, and it trains"""
    import yolox.core.trainer
    import yolox.utils
    from yolox.exp import get_exp
    monkeypatch.setattr(ops, 'VERIFY_SMALL_INT', False)      # the suite's tag check reads the device: not inside a capture
    for module in (yolox.utils, yolox.core.trainer):
        monkeypatch.setattr(module, 'get_rank', lambda: 0)
        monkeypatch.setattr(module, 'get_world_size', lambda: 2)
    exp = get_exp(None, 'e-yolox-s')
    exp.merge(['T', '3', 'embedding', 'arsnn', 'num_classes', '2', 'spike_attach', 'True', 'thresh', '1', 'readout', 'sum', 'embedding_depth', '2',
               'embedding_ksize', '5', 'write_zero', 'True', 'spike_fn', 'atan'] + ['use_spike', 'True', 'input_size', '(64, 64)', 'test_size', '(64, 64)'])
    exp.max_epoch, exp.print_interval, exp.output_dir = 1, 1, str(tmp_path)
    exp.train_input, exp.store_recordings, exp.store_shard = 'dat_store', (2, 8, 3000), 'recordings'
    torch.manual_seed(5)
    tr = exp.get_trainer(types.SimpleNamespace(batch_size=8, fp16=False, experiment_name='store_ranks', ckpt=None, resume=False))
    tr.train()
    loader = tr.train_loader
    assert tr.is_distributed and isinstance(loader, data.Gen1StoreLoader) and loader.sharded and (loader.rank, loader.world, loader.batch_size) == (0, 2, 4)
    assert loader.store.shard == (0, 2) and len(loader.store) == 16 and len(loader.store.owned_samples) == 8
    assert len(loader) == tr.max_iter == 2 and loader.epoch == 1
    assert len(tr.log) == 2 and all(np.isfinite(r['loss']) for r in tr.log)
    assert tr.exchange is None or not tr.exchange.bound
    torch.cuda.set_stream(torch.cuda.default_stream())
