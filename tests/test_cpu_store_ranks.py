"""CPU-only tests of store training on N ranks: the replica rule of the three store loaders (a rank's batch is rows ``rank::world`` of the
single-process batch), ``data.shard_recordings`` and its balance bound, the tables of sharded stores against the unsharded ones, the
draws of the loaders over a sharded store, the index guard, and the experiment's wiring.  Everything compared here is an integer table
or a draw: every comparison is exact."""
import os
import types

import numpy as np
import pytest
import torch

from eas_snn_amd import data

SENSOR, CANVAS = (24, 32), (32, 64)


def small_exp(**kw):
    return types.SimpleNamespace(Tm=3, Tl=1, input_size=CANVAS, test_size=CANVAS, num_classes=2, window=-20, **kw)


def gen1_recs(n_files=3, seed=3):
    # recordings of different sizes (500 .. 3000 events), so that the weights of the greedy assignment differ
    return [data.synth_gen1_recordings(f + 1, 6, n_events=500 + 1250 * f, sensor_hw=SENSOR, seed=seed)[f] for f in range(n_files)]


def gen4_recs(n_files=3):
    return data.synth_gen4_recordings(n_files, 12, (12, 16), 10, 3, seed=4)


def atis_recs(n_files=12):
    return data.synth_ncaltech_recordings(n_files, 3000, sensor_hw=SENSOR, seed=5)


def gen1_store(**kw):
    return data.Gen1Store(gen1_recs(), 1, (-20_000, 0), 'cpu', sensor_hw=SENSOR, **kw)


def gen4_store(**kw):
    return data.Gen4Store(gen4_recs(), 3, 'cpu', sensor_hw=(12, 16), nbins=10, **kw)


def atis_store(**kw):
    return data.NCaltechStore(atis_recs(), 1, None, 'cpu', sensor_hw=SENSOR, **kw)


KINDS = {'gen1': (gen1_store, data.Gen1StoreLoader), 'gen4': (gen4_store, data.Gen4StoreLoader), 'atis': (atis_store, data.NCaltechStoreLoader)}


def kind_exp(kind):
    return types.SimpleNamespace(Tm=3, Tl=1, input_size=(32, 32) if kind == 'gen4' else CANVAS, test_size=CANVAS, num_classes=3, window=-20)


# ------------------------------------------------------------------------------------------------ 1. replica mode
@pytest.mark.parametrize('kind', sorted(KINDS))
@pytest.mark.parametrize('world', [2, 3])
def test_rank_batches_are_the_rows_of_the_single_process_batch(kind, world):
    build, Loader = KINDS[kind]
    store, exp, b = build(), kind_exp(kind), 2
    single = Loader(exp, b * world, store=store, seed=7)
    ranks = [Loader(exp, b, store=store, seed=7, rank=r, world=world) for r in range(world)]
    assert len(single) == len(store) // (b * world) >= 1 and all(len(ld) == len(single) for ld in ranks)
    for epoch in (0, 1):
        whole = single.batches(epoch)
        seen = []
        for r, ld in enumerate(ranks):
            mine = ld.batches(epoch)
            assert len(mine) == len(whole)
            for got, want in zip(mine, whole):
                assert len(got) == len(want) == (2 if kind == 'atis' else 3)
                for g, w in zip(got, want):
                    assert g.dtype == w.dtype and g.shape == (b,) + w.shape[1:] and np.array_equal(g, w[r::world])      # (P too)
                seen += got[0].tolist()
        assert len(seen) == len(set(seen)) == len(single) * b * world             # no sample twice across the ranks of an epoch
    assert not np.array_equal(single.batches(0)[0][0], single.batches(1)[0][0])


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_rank_0_of_a_world_of_1_is_the_loader_of_before(kind):
    build, Loader = KINDS[kind]
    store, exp = build(), kind_exp(kind)
    plain, one = Loader(exp, 4, store=store, seed=2), Loader(exp, 4, store=store, seed=2, rank=0, world=1)
    assert len(plain) == len(one) == len(store) // 4 and not plain.sharded
    # today's rule, written out: the state of (seed, epoch), a permutation of all samples, the batch taken in order
    order = np.random.RandomState((2 * 1_000_003 + 1) % (1 << 32)).permutation(len(store))
    for a, b in zip(plain.batches(1), one.batches(1)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(np.concatenate([d[0] for d in plain.batches(1)]), order[:len(plain) * 4])
    with pytest.raises(ValueError):
        Loader(exp, 4, store=store, rank=2, world=2)


# ------------------------------------------------------------------------------------------------ 2. shard_recordings
def loads(names, weights, ranks, world):
    out = [0] * world
    for n, w in zip(names, weights):
        out[ranks[n]] += w
    return out


@pytest.mark.parametrize('weights', [[5] * 8, [5] * 7, [1000, 3, 2, 2, 1], [9, 8, 7, 6, 5, 4, 3, 2, 1, 0], [4, 4], [7], [0, 0, 0], [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5]])
@pytest.mark.parametrize('world', [1, 2, 3, 4, 8])
def test_shard_recordings_deals_every_recording_once_within_the_bound(weights, world):
    names = [f'rec{i}' for i in range(len(weights))]
    ranks = data.shard_recordings(names, weights, world)
    assert sorted(ranks) == sorted(names) and all(isinstance(r, int) and 0 <= r < world for r in ranks.values())
    assert ranks == data.shard_recordings(list(names), tuple(weights), world)                   # a function of its arguments
    load = loads(names, weights, ranks, world)
    assert sum(load) == sum(weights) and max(load) - min(load) <= max(weights)
    assert max(load) <= sum(weights) / world + max(weights)
    if world == 1:
        assert set(ranks.values()) == {0}
    if world > len(weights) and min(weights) > 0:
        assert sorted(ranks.values()) == list(range(len(weights)))                              # more ranks than recordings: one each


def test_shard_recordings_order_and_ties():
    assert data.shard_recordings('abcd', [1, 1, 1, 1], 2) == {'a': 0, 'b': 1, 'c': 0, 'd': 1}    # ties: the order given, the lower rank
    assert data.shard_recordings('abc', [1, 5, 2], 2) == {'b': 0, 'c': 1, 'a': 1}                 # descending weight
    assert data.shard_recordings([], [], 3) == {}
    for bad in ((['a', 'a'], [1, 2], 2), (['a'], [1, 2], 2), (['a'], [1], 0)):
        with pytest.raises(ValueError):
            data.shard_recordings(*bad)


# ------------------------------------------------------------------------------------------------ 3. sharded tables
def same_label_side(shard, whole, tables):
    assert len(shard) == len(whole) and shard.sample_names == whole.sample_names
    for k in tables:
        assert np.array_equal(shard.host[k], whole.host[k]) and shard.host[k].dtype == whole.host[k].dtype, k
        assert torch.equal(getattr(shard, k), getattr(whole, k)), k
    for i in range(len(whole)):
        assert np.array_equal(shard.raw_labels(i), whole.raw_labels(i))


@pytest.mark.parametrize('world', [2, 3])
def test_gen1_shards_keep_every_label_and_their_own_records(world):
    recs, whole = gen1_recs(), gen1_store()
    assert whole.owned_samples.tolist() == list(range(len(whole))) and whole.owns([0, len(whole) - 1]).all() and not whole.sharded
    assert whole.shard is None and whole.sample_rank is None
    ranks = data.shard_recordings([r[0] for r in recs], [len(r[1]) for r in recs], world)
    owned_all, held = [], 0
    for r in range(world):
        shard = gen1_store(shard=(r, world))
        same_label_side(shard, whole, ('boxes', 'group_start', 'group_t', 'group_file'))
        assert shard.shard == (r, world) and shard.sharded and np.array_equal(shard.group_rows, whole.group_rows)
        mine = [n for n in whole.names if ranks[n] == r]
        assert np.array_equal(shard.sample_rank, np.array([ranks[whole.names[f]] for f in whole.host['group_file']]))
        assert shard.owned_samples.dtype == np.int64 and (np.diff(shard.owned_samples) > 0).all()
        assert shard.owned_samples.tolist() == [i for i, f in enumerate(whole.host['group_file']) if whole.names[f] in mine]
        assert shard.owns(shard.owned_samples).all() and shard.owns(np.arange(len(whole))).sum() == len(shard.owned_samples)
        assert not shard.owns([-1, len(whole)]).any()
        # the record areas of the owned recordings back to back, a zero-length area for the others
        sizes = np.diff(shard.host['file_offsets'])
        assert [int(s) for s in sizes] == [int(s) if whole.names[f] in mine else 0 for f, s in enumerate(np.diff(whole.host['file_offsets']))]
        parts = [whole.records[8 * whole.host['file_offsets'][f]:8 * whole.host['file_offsets'][f + 1]] for f, n in enumerate(whole.names) if n in mine]
        assert torch.equal(shard.records, torch.cat(parts) if parts else torch.zeros(0, dtype=torch.uint8))
        owned_all += shard.owned_samples.tolist()
        held += shard.records.numel()
        # the same store from owned=, the heavy member of the others None
        again = data.Gen1Store([(n, dat if n in mine else None, rows) for n, dat, rows in recs], 1, (-20_000, 0), 'cpu', sensor_hw=SENSOR, owned=mine)
        same_label_side(again, whole, ('boxes', 'group_start', 'group_t', 'group_file'))
        assert torch.equal(again.records, shard.records) and np.array_equal(again.owned_samples, shard.owned_samples)
        assert again.shard is None and again.sample_rank is None and again.sharded == (len(mine) < len(recs))
    assert sorted(owned_all) == list(range(len(whole))) and held == whole.records.numel()
    with pytest.raises(ValueError):
        gen1_store(shard=(world, world))
    with pytest.raises(ValueError):
        gen1_store(shard=(0, world), owned=['x'])


@pytest.mark.parametrize('world', [2, 3])
def test_gen4_shards_keep_every_label_and_their_own_representations(world):
    recs, whole = gen4_recs(), gen4_store()
    assert whole.owned_samples.tolist() == list(range(len(whole))) and not whole.sharded
    assert whole.held_first is whole.group_first and whole.held_lo is whole.group_lo
    assert np.array_equal(whole.held_offsets, whole.host['rep_offsets'])
    ranks = data.shard_recordings([r[0] for r in recs], [len(r[1]) for r in recs], world)
    owned_all = []
    for r in range(world):
        shard = gen4_store(shard=(r, world))
        tables = ('boxes', 'group_start', 'group_first', 'group_lo', 'rep_offsets')
        same_label_side(shard, whole, tables)
        mine = [n for n in whole.names if ranks[n] == r]
        file_of = whole.group_file
        assert shard.owned_samples.tolist() == [i for i, f in enumerate(file_of) if whole.names[f] in mine]
        assert np.diff(shard.held_offsets).tolist() == [12 if n in mine else 0 for n in whole.names]
        # what frames gathers: the sample's first representation relative to its recording is the unsharded store's, at the recording's
        # place in this rank's sums; a sample that is not owned lies wholly in front of its (empty) recording
        own = shard.owns(np.arange(len(whole)))
        first, lo = shard.held_first.numpy(), shard.held_lo.numpy()
        assert np.array_equal((first - lo)[own], (whole.host['group_first'] - whole.host['group_lo'])[own])
        assert np.array_equal(lo[own], shard.held_offsets[:-1][file_of][own])
        assert (first[~own] == -3).all() and (lo[~own] == 0).all()
        assert (first[own] + 3 <= shard.held_offsets[1:][file_of][own]).all()            # the last slice lies inside the recording
        owned_all += shard.owned_samples.tolist()
        again = data.Gen4Store([(rec[0], rec[1] if rec[0] in mine else None) + rec[2:] for rec in recs], 3, 'cpu', sensor_hw=(12, 16), owned=mine)
        same_label_side(again, whole, ('boxes', 'group_start'))
        assert np.array_equal(again.owned_samples, shard.owned_samples) and torch.equal(again.held_first, shard.held_first)
        # a recording passed as None counts objframe_idx_2_repr_idx[-1] + 1 representations (11 of the 12 here)
        assert np.diff(again.host['rep_offsets']).tolist() == [12 if n in mine else 11 for n in whole.names]
    assert sorted(owned_all) == list(range(len(whole)))


def test_ncaltech_shards_keep_every_box_and_their_own_records():
    recs, whole = atis_recs(), atis_store()
    world = 3
    ranks = data.shard_recordings(whole.sample_names, [len(r[2]) for r in recs], world)
    owned_all, held = [], 0
    for r in range(world):
        shard = atis_store(shard=(r, world))
        same_label_side(shard, whole, ('boxes', 'group_start'))
        assert shard.class_names == whole.class_names
        mine = [i for i, n in enumerate(whole.sample_names) if ranks[n] == r]
        assert shard.owned_samples.tolist() == mine and np.array_equal(shard.sample_rank, [ranks[n] for n in whole.sample_names])
        sizes = np.diff(whole.host['file_offsets'])
        assert np.diff(shard.host['file_offsets']).tolist() == [int(sizes[i]) if i in mine else 0 for i in range(len(whole))]
        assert shard.max_file_records == max(int(sizes[i]) for i in mine)
        again = data.NCaltechStore([(c, s, rec if f'{c}-{s}' in {whole.sample_names[i] for i in mine} else None, ann) for c, s, rec, ann in recs],
                                   1, None, 'cpu', sensor_hw=SENSOR, owned=[whole.sample_names[i] for i in mine])
        assert torch.equal(again.records, shard.records) and again.class_names == whole.class_names
        owned_all += mine
        held += shard.records.numel()
        assert shard.records.numel() <= whole.records.numel() / world + 5 * sizes.max()
    assert sorted(owned_all) == list(range(len(whole))) and held == whole.records.numel()


def write_gen1_dir(path, recs):
    os.makedirs(path)
    for name, dat, rows in recs:
        np.asarray(dat, dtype=np.uint8).tofile(os.path.join(path, name + '_td.dat'))
        np.save(os.path.join(path, name + '_bbox.npy'), rows)


def test_gen1_shard_from_directories_opens_only_its_own_recordings(tmp_path):
    recs = gen1_recs()
    write_gen1_dir(str(tmp_path / 'train'), recs[:2])
    write_gen1_dir(str(tmp_path / 'val'), recs[2:])
    dirs = [str(tmp_path / 'train'), str(tmp_path / 'val')]
    whole = data.Gen1Store.from_directories(dirs, 1, (-20_000, 0), 'cpu', sensor_hw=SENSOR)
    assert whole.names == [r[0] for r in recs] and not whole.sharded
    ranks = data.shard_recordings([r[0] for r in recs], [len(r[1]) for r in recs], 2)        # the file is the byte image: its size is len()
    asked_all = []
    for r in range(2):
        asked = []

        def read(path):
            asked.append(os.path.basename(path)[:-len('_td.dat')])
            return np.fromfile(path, dtype=np.uint8)
        shard = data.Gen1Store.from_directories(dirs, 1, (-20_000, 0), 'cpu', sensor_hw=SENSOR, shard=(r, 2), read_dat=read)
        assert asked == [n for n in whole.names if ranks[n] == r] and len(asked) >= 1
        same_label_side(shard, whole, ('boxes', 'group_start', 'group_t', 'group_file'))
        assert shard.shard == (r, 2) and np.array_equal(shard.sample_rank, [ranks[whole.names[f]] for f in whole.host['group_file']])
        mem = gen1_store(shard=(r, 2))
        assert torch.equal(shard.records, mem.records) and np.array_equal(shard.owned_samples, mem.owned_samples)
        asked_all += asked
    assert sorted(asked_all) == sorted(whole.names)


def test_gen4_shard_from_directories_opens_only_its_own_representations(tmp_path):
    recs = gen4_recs()
    reps = {}
    for name, rep, obj2repr, rows, obj2label, times in recs:
        label_dir, rep_dir = tmp_path / 'train' / name / 'labels_v2', tmp_path / 'train' / name / 'event_representations_v2' / data.GEN4_REP_NAME
        os.makedirs(label_dir)
        os.makedirs(rep_dir)
        np.savez(label_dir / 'labels.npz', labels=rows, objframe_idx_2_label_idx=obj2label)
        np.save(label_dir / 'timestamps_us.npy', times)
        np.save(rep_dir / 'objframe_idx_2_repr_idx.npy', obj2repr)
        reps[str(rep_dir)] = rep
    whole = gen4_store()
    ranks = data.shard_recordings([r[0] for r in recs], [int(r[2][-1]) + 1 for r in recs], 2)
    asked_all = []
    for r in range(2):
        asked = []

        def read(rep_dir):
            asked.append(os.path.basename(os.path.dirname(os.path.dirname(rep_dir))))
            return reps[rep_dir]
        shard = data.Gen4Store.from_directories(str(tmp_path / 'train'), 3, 'cpu', sensor_hw=(12, 16), read_representations=read, shard=(r, 2))
        assert asked == [n for n in whole.names if ranks[n] == r] and len(asked) >= 1
        same_label_side(shard, whole, ('boxes', 'group_start'))
        assert shard.shard == (r, 2) and shard.owned_samples.tolist() == [i for i, f in enumerate(whole.group_file) if whole.names[f] in asked]
        asked_all += asked
    assert sorted(asked_all) == sorted(whole.names)


def test_ncaltech_shard_from_directory_opens_only_its_own_recordings(tmp_path):
    recs = atis_recs(6)
    lines = []
    for c, stem, rec, ann in recs:
        os.makedirs(tmp_path / 'Caltech101' / c, exist_ok=True)
        os.makedirs(tmp_path / 'Caltech101_annotations' / c, exist_ok=True)
        np.asarray(rec, dtype=np.uint8).tofile(tmp_path / 'Caltech101' / c / (stem + '.bin'))
        np.asarray(ann, dtype=np.uint8).tofile(tmp_path / 'Caltech101_annotations' / c / ('annotation_' + stem + '.bin'))
        lines.append(f'Caltech101/{c}/{stem}.bin Caltech101_annotations/{c}/annotation_{stem}.bin\n')
    (tmp_path / 'train.txt').write_text(''.join(lines))
    whole = data.NCaltechStore.from_directory(str(tmp_path), 'train', 1, None, 'cpu', sensor_hw=SENSOR)
    ranks = data.shard_recordings(whole.sample_names, [len(r[2]) for r in recs], 2)
    for r in range(2):
        asked = []

        def read(path):
            asked.append(os.path.basename(path))
            return np.fromfile(path, dtype=np.uint8)
        shard = data.NCaltechStore.from_directory(str(tmp_path), 'train', 1, None, 'cpu', sensor_hw=SENSOR, shard=(r, 2), read_bin=read)
        mine = [i for i, n in enumerate(whole.sample_names) if ranks[n] == r]
        assert asked == [recs[i][1] + '.bin' for i in mine] and shard.owned_samples.tolist() == mine and shard.shard == (r, 2)
        same_label_side(shard, whole, ('boxes', 'group_start'))
        assert shard.class_names == whole.class_names


# ------------------------------------------------------------------------------------------------ 4. loaders over a sharded store
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_shard_loaders_draw_their_own_samples(kind):
    build, Loader = KINDS[kind]
    exp, world, b = kind_exp(kind), 2, 2
    stores = [build(shard=(r, world)) for r in range(world)]
    loaders = [Loader(exp, b, store=s, seed=3) for s in stores]
    counts = [len(s.owned_samples) for s in stores]
    assert sum(counts) == len(stores[0]) and min(counts) >= b
    assert all(ld.sharded and (ld.rank, ld.world) == (r, world) and len(ld) == min(counts) // b for r, ld in enumerate(loaders))
    for r, (ld, s) in enumerate(zip(loaders, stores)):
        for epoch in (0, 1):
            draws = ld.batches(epoch)
            idx = np.concatenate([d[0] for d in draws])
            assert len(draws) == len(ld) and all(d[0].shape == (b,) and d[0].dtype == np.int64 for d in draws)
            assert s.owns(idx).all() and len(set(idx.tolist())) == len(idx)
            again = Loader(exp, b, store=s, seed=3).batches(epoch)
            assert all(np.array_equal(x, y) for d, e in zip(draws, again) for x, y in zip(d, e))              # (seed, epoch, rank) alone
        params = [np.concatenate([d[1] for d in ld.batches(e)]) for e in (0, 1)]
        assert not np.array_equal(params[0], params[1])                                                    # epochs differ
        assert not np.array_equal(params[0], np.concatenate([d[1] for d in Loader(exp, b, store=s, seed=4).batches(0)]))
    p0, p1 = (np.concatenate([d[1] for d in ld.batches(0)]) for ld in loaders)
    assert not np.array_equal(p0, p1)                                                                      # ranks differ
    # the random state is the documented one, and the draws come in today's per-sample order
    rs = data._shard_state(3, 1, 1)
    order = stores[1].owned_samples[rs.permutation(counts[1])]
    first = loaders[1].batches(1)[0]
    assert np.array_equal(first[0], order[:b])
    (H, W), (Hc, Wc) = stores[1].sensor_hw, exp.input_size
    for row, s in enumerate(order[:b]):
        assert tuple(first[1][row]) == tuple(data.jitter_params(H, W, Hc, Wc, jitter=.1 if kind == 'atis' else .3, rng=rs))
        if kind != 'atis':
            n = int(stores[1].group_rows[s])
            assert np.array_equal(first[2][row, :n], rs.permutation(n))


def test_shard_state_is_a_function_of_seed_epoch_and_rank():
    seen = set()
    for seed in (0, 1, 1 << 32):
        for epoch in (0, 1, 2):
            for rank in (0, 1, 2):
                a, b = data._shard_state(seed, epoch, rank).randint(1 << 30, size=4), data._shard_state(seed, epoch, rank).randint(1 << 30, size=4)
                assert np.array_equal(a, b)
                seen.add((seed % (1 << 32), tuple(a)))
    assert len({v for _, v in seen}) == 18 and len(seen) == 18                   # 2 distinct seeds mod 2^32 x 3 epochs x 3 ranks


def test_shard_loader_length_is_the_smallest_rank_and_a_starved_rank_raises():
    exp = small_exp()
    # three recordings of 6 labels on two ranks: 12 and 6 samples
    stores = [gen1_store(shard=(r, 2)) for r in range(2)]
    counts = sorted(len(s.owned_samples) for s in stores)
    assert counts == [6, 12]
    for b, want in ((2, 3), (3, 2), (4, 1), (6, 1)):
        assert [len(data.Gen1StoreLoader(exp, b, store=s)) for s in stores] == [want, want]
    for s in stores:                                             # every rank learns of the starved one, from the tables alone
        with pytest.raises(ValueError, match=r'rank \d owns 6 samples'):
            data.Gen1StoreLoader(exp, 7, store=s)
    # more ranks than recordings: rank 3 owns nothing
    with pytest.raises(ValueError, match='rank 3 owns 0 samples'):
        data.Gen1StoreLoader(exp, 1, store=gen1_store(shard=(3, 4)))
    # a store built from owned= knows its own count only
    part = gen1_store(owned=[gen1_recs()[0][0]])
    assert part.sharded and len(data.Gen1StoreLoader(exp, 4, store=part, rank=1, world=2)) == 1
    with pytest.raises(ValueError, match='rank 1 owns 6 samples'):
        data.Gen1StoreLoader(exp, 7, store=part, rank=1, world=2)


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_an_index_that_is_not_owned_raises_before_anything_is_uploaded(kind, monkeypatch):
    build, Loader = KINDS[kind]
    exp = kind_exp(kind)
    store = build(shard=(0, 2))
    foreign = np.setdiff1d(np.arange(len(store)), store.owned_samples)
    assert len(foreign) >= 1
    with pytest.raises(IndexError, match='not held'):
        store.check_owned([int(store.owned_samples[0]), int(foreign[0])])
    store.check_owned(store.owned_samples)
    monkeypatch.setattr(store, 'frames', lambda *a, **k: pytest.fail('frames was asked for a sample that is not owned'))
    ld = Loader(exp, 2, store=store)
    draws = ld.batches(0)
    draws[0][0][1] = foreign[0]
    monkeypatch.setattr(ld, 'batches', lambda epoch: draws)
    with pytest.raises(IndexError):
        next(iter(ld))
    Eval = {'gen1': data.Gen1StoreEvalLoader, 'gen4': data.Gen4StoreEvalLoader, 'atis': data.NCaltechStoreEvalLoader}[kind]
    with pytest.raises(IndexError):
        Eval(exp, 2, [int(foreign[0])], store)
    with pytest.raises(IndexError):
        Eval(exp, 2, [len(store)], build())
    ok = Eval(exp, 2, store.owned_samples.tolist(), store, min_batches=len(store))
    assert len(ok) == len(store) and len(Eval(exp, 2, store.owned_samples.tolist(), store)) == (len(store.owned_samples) + 1) // 2


# ------------------------------------------------------------------------------------------------ 5. the experiment
def store_exp(train_input, monkeypatch, rank=1, world=2):
    import yolox.utils
    from yolox.exp import get_exp
    monkeypatch.setattr(yolox.utils, 'get_rank', lambda: rank)
    monkeypatch.setattr(yolox.utils, 'get_world_size', lambda: world)
    e = get_exp(None, 'e-yolox-s')
    e.train_input = train_input
    e.store_recordings, e.atis_store_recordings = {'dat_store': (3, 6, 2000), 'hist_store': (3, 12)}.get(train_input, (3, 6, 2000)), (12, 3000)
    e.merge(['input_size', '(32, 32)', 'test_size', '(32, 32)', 'num_classes', '2', 'Tm', '3'])
    return e


@pytest.mark.parametrize('train_input', ['dat_store', 'hist_store', 'atis_store'])
def test_experiment_hands_rank_and_world_to_the_store_loaders(train_input, monkeypatch):
    e = store_exp(train_input, monkeypatch)
    Loader = {'dat_store': data.Gen1StoreLoader, 'hist_store': data.Gen4StoreLoader, 'atis_store': data.NCaltechStoreLoader}[train_input]
    B = 4
    loader = e.get_data_loader(B, True)
    assert type(loader) is Loader and (loader.rank, loader.world, loader.batch_size) == (1, 2, 2) and not loader.sharded
    store = loader.store
    assert not store.sharded and len(store.owned_samples) == len(store)
    # max_iter as the Trainer computes it: the steps of an epoch of the global batch
    assert len(loader) == len(store) // B
    single = Loader(e, B, store=store)
    for got, want in zip(loader.batches(0), single.batches(0)):
        assert all(np.array_equal(g, w[1::2]) for g, w in zip(got, want))
    with pytest.raises(ValueError, match='multiple of the world size'):
        e.get_data_loader(5, True)
    # not distributed: the loader of before, whatever the launcher says
    plain = e.get_data_loader(B, False)
    assert (plain.rank, plain.world, plain.batch_size) == (0, 1, B) and plain.store is store
    # replica evaluation stays rank, rank + world, ... with wrap-around
    ev = e.get_eval_loader(2, True)
    n = len(ev.dataset)
    assert ev.indices == [(1 + 2 * k) % n for k in range((n + 1) // 2)] and ev.batch_size == 2 and ev.min_batches == 0


@pytest.mark.parametrize('train_input', ['dat_store', 'hist_store', 'atis_store'])
def test_experiment_shards_the_stores_when_asked(train_input, monkeypatch):
    import yolox.utils
    e = store_exp(train_input, monkeypatch)
    whole = e.get_data_loader(4, True).store
    e.store_shard = 'recordings'
    loader = e.get_data_loader(4, True)
    store = loader.store
    assert store is not whole and store.shard == (1, 2) and store.sharded and loader.sharded and (loader.rank, loader.world) == (1, 2)
    assert 0 < len(store.owned_samples) < len(store) == len(whole) and store.sample_names == whole.sample_names
    other = len(store) - len(store.owned_samples)
    assert len(loader) == min(other, len(store.owned_samples)) // 2
    assert e.get_data_loader(4, True).store is store                             # kept per (split, rank, world, store_shard)
    # evaluation: the rank's own samples of the test store, ascending, each once
    ev = e.get_eval_loader(2, True)
    assert ev.store.shard == (1, 2) and ev.indices == ev.store.owned_samples.tolist() and ev.batch_size == 2 and ev.min_batches == 0
    monkeypatch.setattr(yolox.utils, 'get_rank', lambda: 0)
    ev0 = e.get_eval_loader(2, True)
    assert ev0.store is not ev.store and sorted(ev0.indices + ev.indices) == list(range(len(ev.dataset)))
    assert e.get_data_loader(4, True).store.shard == (0, 2)
    e.store_shard = 'none'
    assert e.get_data_loader(4, True).store.shard is None
    e.store_shard = 'bogus'
    with pytest.raises(ValueError, match='store_shard'):
        e.get_data_loader(4, True)
    with pytest.raises(ValueError, match='store_shard'):
        e.get_eval_loader(2, True)


def test_evaluators_that_meet_per_batch_get_loaders_of_one_length(monkeypatch):
    """PSEEEvaluator gathers once per batch: the loaders of a sharded evaluation are padded to the longest rank's, with empty batches"""
    import yolox.utils
    from yolox.evaluators import EventEvaluator
    from yolox.evaluators.psee_evaluator import PSEEEvaluator
    e = store_exp('dat_store', monkeypatch)
    e.store_shard, e.data_name = 'recordings', 'gen1'
    assert type(e.get_evaluator(2, True)) is EventEvaluator and e.get_evaluator(2, True).dataloader.min_batches == 0
    e.eval_proph = True
    lengths, owned = [], []
    for rank in (0, 1):
        monkeypatch.setattr(yolox.utils, 'get_rank', lambda: rank)
        ev = e.get_evaluator(2, True)
        assert type(ev) is PSEEEvaluator
        lengths.append(len(ev.dataloader))
        owned.append(len(ev.dataloader.indices))
    assert sorted(owned) == [6, 12] and lengths == [6, 6]                        # batches of 2: 12 samples are 6 batches
    # without a sharded store nothing is padded
    e.store_shard = 'none'
    assert e.get_evaluator(2, True).dataloader.min_batches == 0


class _ToyModel(torch.nn.Module):
    """a fixed decoded head output on the CPU, whatever the frames"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))

    def forward(self, x):
        out = torch.zeros(x.shape[0], 4, 7)
        for a in range(4):
            out[:, a, 0], out[:, a, 1] = 12. + 10 * a, 10. + 3 * a
            out[:, a, 2:4] = 14.
            out[:, a, 4] = 0.9 * self.w
            out[:, a, 5 + a % 2] = 0.8
        return out


@pytest.mark.parametrize('which', ['event', 'psee'])
def test_an_evaluation_padded_with_empty_batches_equals_the_unpadded_one(which, monkeypatch):
    import yolox.evaluators.event_evaluator as EV
    from yolox.evaluators.psee_evaluator import PSEEEvaluator
    from oracle import postprocess_ref

    def cpu_postprocess(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, class_agnostic=False):
        out = postprocess_ref.postprocess(prediction.cpu().numpy(), num_classes, conf_thre, nms_thre, class_agnostic)
        return [None if o is None else torch.from_numpy(o) for o in out]
    monkeypatch.setattr(EV, 'postprocess', cpu_postprocess)
    exp, store = small_exp(), gen1_store(shard=(0, 2))
    monkeypatch.setattr(store, 'frames', lambda idx, par, exp, canvas_hw=None: torch.zeros((len(idx), 1, 3, 2) + tuple(canvas_hw)))
    runs = []
    for pad in (0, 5):
        loader = data.Gen1StoreEvalLoader(exp, 4, store.owned_samples.tolist(), store, min_batches=pad)
        batches = list(loader)
        assert len(batches) == len(loader) == max(pad, 2) and [len(b[3]) for b in batches] == [4, 2] + [0] * (len(batches) - 2)
        for frames, labels, (hs, ws), ids in batches[2:]:
            assert frames.shape == (0, 1, 3, 2) + CANVAS and labels == [] and len(hs) == len(ws) == 0 and ids.dtype == torch.int64
        if which == 'psee':
            ev = PSEEEvaluator(loader, CANVAS, 0.3, 0.5, 2, dataset='gen1')
        else:
            ev = EV.EventEvaluator(loader, CANVAS, 0.3, 0.5, 2)
        (ap, ap50, summary), outputs = ev.evaluate(_ToyModel(), return_outputs=True)
        runs.append((ap, ap50, outputs if which == 'event' else [o.tolist() for o in outputs]))
    assert runs[0] == runs[1] and len(runs[0][2]) == 6
    if which == 'event':
        assert sorted(runs[0][2]) == store.owned_samples.tolist()                # every owned sample once, under its global id
