"""GPU tests of the Gen1 store that keeps only the records its samples read: ``ops.records_gather`` against numpy, bit for bit, with
canary records around the destination span; ``ops.record_ranges_union`` against the numpy checker (tests/window_store_ref.py, compared
with a per-record mask by test_cpu_window_store.py); ``data.Gen1WindowStore`` against the full ``Gen1Store`` on the same recordings --
frames, targets, loaders, a captured graph -- and the memory its build takes.  Everything is a copy or index work: every comparison is
exact."""
import gc
import os
import types

import numpy as np
import pytest
import torch

import window_store_ref as ref
from eas_snn_amd import _lib, data, ops

pytestmark = pytest.mark.gpu

TILE, WAVE_TILE = 4096, 1024           # destination records per block and per wave of eas_records_gather (csrc/records.hip)
CANVAS, TM = (64, 96), 4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ the gather
def run_gather(dev, n_src, segments, dst_offset, tail=3, seed=0):
    """the op and the checker on the same inputs: the whole destination, canaries in front of and behind the span included, must agree"""
    rng = np.random.default_rng(seed)
    segments = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
    seg_dst = np.r_[0, np.cumsum(segments[:, 1] - segments[:, 0])].astype(np.int64)
    src = rng.integers(0, 2 ** 32, size=(n_src, 2), dtype=np.uint32)
    dst = np.full((dst_offset + int(seg_dst[-1]) + tail, 2), 0xA5A5A5A5, dtype=np.uint32)
    want = ref.gather(src, segments, seg_dst, dst, dst_offset)
    d = torch.from_numpy(dst.view(np.uint8).reshape(-1)).to(dev)
    n = ops.records_gather(torch.from_numpy(src.view(np.uint8).reshape(-1)).to(dev), torch.from_numpy(segments).to(dev),
                           torch.from_numpy(seg_dst).to(dev), d, dst_offset)
    got = d.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert n == seg_dst[-1] and np.array_equal(got, want)
    assert (got[:dst_offset] == 0xA5A5A5A5).all() and (got[dst_offset + n:] == 0xA5A5A5A5).all()
    return got


@pytest.mark.parametrize('src_start', [0, 1, 6, 7])
@pytest.mark.parametrize('dst_offset', [0, 1, 4, 5])
def test_gather_one_segment_every_parity(dev, src_start, dst_offset):
    """S = 1; source and destination starts even and odd: equal parity takes the 16-byte path (with and without a single record in front
    and behind), unequal parity the 8-byte path; lengths around a lane pair, a wave round, the wave tile and the block tile"""
    for n in (1, 2, 3, 127, 128, 129, WAVE_TILE - 1, WAVE_TILE + 2, TILE + 1, 2 * TILE + WAVE_TILE + 77):
        run_gather(dev, src_start + n + 5, [(src_start, src_start + n)], dst_offset, seed=n)


def test_gather_three_hundred_short_segments(dev):
    rng = np.random.default_rng(3)
    a = np.cumsum(rng.integers(1, 6, 300))                                       # sorted starts, 0 .. 4 records between two segments
    length = rng.integers(1, 4, 300)
    a = a + np.r_[0, np.cumsum(length)[:-1]]
    segments = np.stack([a, a + length], 1)
    for dst_offset in (0, 3):
        run_gather(dev, int(segments[-1, 1]) + 2, segments, dst_offset)
    run_gather(dev, int(segments[-1, 1]) + 2, segments[rng.permutation(300)], 7)                      # the source order is free


def test_gather_segments_across_tiles(dev):
    """segments that cross the boundary of a wave's and of a block's tile at either parity, a total that is no multiple of the tile, an odd
    offset; thousands of short segments over several tiles"""
    segs = [(10, 10 + WAVE_TILE - 3), (5000, 5000 + 7), (20_001, 20_001 + TILE), (9, 9 + 2 * TILE + 1), (40_000, 40_000 + 31)]
    for dst_offset in (0, 1, TILE - 1):
        got = run_gather(dev, 50_000, segs, dst_offset)
        assert (len(got) - dst_offset - 3) % TILE != 0
    rng = np.random.default_rng(5)
    many = np.sort(rng.choice(60_000, 2 * 9000, replace=False)).reshape(-1, 2)                         # 9000 segments of ~3 records
    run_gather(dev, 60_001, many, 5)


def test_gather_more_tiles_than_blocks(dev):
    """8192 blocks at most are launched: with more tiles a block goes on to further ones.  One segment of 8192 tiles and a bit, odd
    starts on both sides, compared on the device."""
    n = 8192 * TILE + 2 * TILE + 5
    src = torch.randint(-2 ** 62, 2 ** 62, (n + 4,), dtype=torch.int64, device=dev)
    dst = torch.full((n + 6,), -1, dtype=torch.int64, device=dev)
    seg = torch.tensor([[3, 3 + n]], dtype=torch.int64, device=dev)
    assert ops.records_gather(src.view(torch.uint8), seg, torch.tensor([0, n], dtype=torch.int64, device=dev), dst.view(torch.uint8), 1) == n
    assert torch.equal(dst[1:1 + n], src[3:3 + n]) and dst[0] == -1 and (dst[1 + n:] == -1).all()


def test_gather_refuses_segments_that_do_not_fit(dev):
    z = lambda n: torch.zeros(8 * n, dtype=torch.uint8, device=dev)             # noqa: E731
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)                # noqa: E731
    for src, seg, seg_dst, dst, off in ((z(10), [[4, 11]], [0, 7], z(20), 0), (z(10), [[4, 9]], [0, 5], z(8), 4), (z(10), [[4, 9]], [0, 4], z(20), 0),
                                        (z(10), [[-1, 3]], [0, 4], z(20), 0), (z(10), [[5, 3]], [0, -2], z(20), 0)):
        with pytest.raises(ValueError):
            ops.records_gather(src, t(seg), t(seg_dst), dst, off)
    assert ops.records_gather(z(10), t([]).reshape(0, 2), t([0]), z(4)) == 0


# ------------------------------------------------------------------------------------------------ the union
@pytest.mark.parametrize('seed,n_records,m,max_len', [(0, 40, 1, None), (1, 40, 12, None), (2, 300, 60, None), (3, 5000, 3000, None), (4, 7, 30, None),
                                                      (5, 2, 9, None), (6, 20_000, 400, 30)])
def test_union_equals_the_checker_and_maps_every_range(dev, seed, n_records, m, max_len):
    ranges = ref.random_ranges(np.random.default_rng(seed), n_records, m, max_len)
    segments, seg_dst, mapped = ops.record_ranges_union(torch.from_numpy(ranges).to(dev))
    want = ref.union(ranges)
    assert segments.dtype == seg_dst.dtype == mapped.dtype == torch.int64 and mapped.shape == ranges.shape
    assert np.array_equal(segments.cpu().numpy(), want[0]) and np.array_equal(seg_dst.cpu().numpy(), want[1])
    got = mapped.cpu().numpy()
    full_rows = ranges[:, 1] > ranges[:, 0]
    assert np.array_equal(got[full_rows], want[2][full_rows])
    assert (got[~full_rows, 0] == got[~full_rows, 1]).all() and (got >= 0).all() and (got <= want[1][-1]).all()
    # compact[mapped[i]] == full[ranges[i]] on records gathered by the kernel
    full = torch.arange(n_records, dtype=torch.int64, device=dev) * 3 + 1
    compact = torch.full((int(seg_dst[-1]),), -1, dtype=torch.int64, device=dev)
    ops.records_gather(full.view(torch.uint8), segments, seg_dst, compact.view(torch.uint8))
    full, compact = full.cpu().numpy(), compact.cpu().numpy()
    for (a, e), (ma, me) in zip(ranges, got):
        assert np.array_equal(compact[ma:me], full[a:e])


def test_union_of_nothing(dev):
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev).reshape(-1, 2)          # noqa: E731
    for ranges in (t([]), t([[4, 4]]), t([[4, 4], [0, 0], [9, 9]])):
        segments, seg_dst, mapped = ops.record_ranges_union(ranges)
        assert segments.shape == (0, 2) and seg_dst.tolist() == [0] and mapped.shape == ranges.shape and not mapped.any()


# ------------------------------------------------------------------------------------------------ the store
@pytest.fixture(scope='module')
def recordings():
    return ref.recordings()


@pytest.fixture(scope='module')
def stores(dev, recordings):
    """{Tl: (the full store -- the oracle, pinned to the reference by the fixtures of its own tests --, the window store, the checker's layout)}"""
    return {Tl: (data.Gen1Store(recordings, Tl, ref.WINDOW, dev), data.Gen1WindowStore(recordings, Tl, ref.WINDOW, dev), ref.layout(recordings, Tl))
            for Tl in (1, 2)}


def exp_for(Tl, aggregation='micro_sum', **kw):
    return types.SimpleNamespace(Tm=TM, Tl=Tl, input_size=CANVAS, test_size=CANVAS, num_classes=2, window=-20, aggregation=aggregation, **kw)


@pytest.mark.parametrize('Tl', [1, 2])
def test_store_keeps_what_the_checker_says(dev, stores, Tl):
    full, win, lay = stores[Tl]
    assert win.total_records == lay['total'] == full.records.numel() // 8 and win.kept_records == lay['kept'] < win.total_records
    assert win.used_bytes == 8 * lay['kept'] == win.records.numel() and win.capacity_bytes >= win.used_bytes
    assert win.file_offsets.tolist() == lay['file_offsets'].tolist() and win.sample_ranges.shape == (len(full), Tl, 2) and len(win) == len(full) == 30
    got, want = win.sample_ranges.cpu().numpy(), lay['sample_ranges']
    some = want[..., 1] > want[..., 0]
    assert np.array_equal(got[some], want[some]) and (got[~some][:, 0] == got[~some][:, 1]).all() and (got >= 0).all() and (got <= lay['kept']).all()
    assert (~some).sum() >= 3 * Tl                                              # the label in the gap, the recording without events
    # the kept records are the records of the full store at the checker's indices, in order
    rows = full.records.view(torch.int64)[torch.from_numpy(lay['keep']).to(dev)]
    assert torch.equal(win.records.view(torch.int64), rows)
    # the parent's tables, names and labels
    assert win.sample_names == full.sample_names and win.names == full.names and win.max_group_rows == full.max_group_rows
    for k in ('boxes', 'group_start', 'group_t', 'group_file'):
        assert torch.equal(getattr(win, k), getattr(full, k))
    assert np.array_equal(win.raw_labels(11), full.raw_labels(11))


@pytest.mark.parametrize('aggregation', ['micro_sum', 'timesurface'])
@pytest.mark.parametrize('Tl', [1, 2])
def test_store_frames_and_targets_equal_the_full_store(dev, stores, Tl, aggregation):
    full, win, _ = stores[Tl]
    exp = exp_for(Tl, aggregation)
    rs = np.random.RandomState(5)
    idx = torch.from_numpy(rs.permutation(len(full)).astype(np.int64)).to(dev)
    par = np.array([data.jitter_params(*ref.SENSOR, *CANVAS, jitter=.3, rng=rs) for _ in range(len(full))], dtype=np.int32)
    assert set(par[:, 4]) == {0, 1}                                             # flipped and not
    par = torch.from_numpy(par).to(dev)
    want, got = full.frames(idx, par, exp), win.frames(idx, par, exp)
    assert got.shape == (30, Tl, TM, 2, *CANVAS) and got.dtype == torch.float32 and torch.equal(got, want)
    filled = want.reshape(30, -1).any(1).cpu().numpy()
    assert filled.sum() == 27 and not filled[np.isin(idx.cpu().numpy(), [14, 22, 23])].any()          # all but the gap label and 'noevents'
    assert torch.equal(win.targets(idx, par, None, CANVAS), full.targets(idx, par, None, CANVAS))
    # every sample alone, too (a batch of one)
    for b in (0, 7, 29):
        assert torch.equal(win.frames(idx[b:b + 1], par[b:b + 1], exp), want[b:b + 1])
    with pytest.raises(ValueError):
        win.frames(idx, par, exp_for(3 - Tl, aggregation))


def test_trim_keeps_the_frames(dev, recordings):
    full, exp = data.Gen1Store(recordings[:2], 1, ref.WINDOW, dev), exp_for(1)
    win = data.Gen1WindowStore(recordings[:2], 1, ref.WINDOW, dev, capacity_bytes=4_000_000)
    idx = torch.arange(len(full), device=dev)
    par = [data.letterbox_params(*ref.SENSOR, *CANVAS)] * len(full)
    assert win.capacity_bytes == 4_000_000 > win.used_bytes and win.trim() is win and win.capacity_bytes == win.used_bytes
    assert win.records.untyped_storage().nbytes() == win.used_bytes
    assert torch.equal(win.frames(idx, par, exp), full.frames(idx, par, exp))


# ------------------------------------------------------------------------------------------------ loaders and capture
def small_exp(store_records):
    return exp_for(1, store_records=store_records, store_recordings=(2, 8, 3000))


def test_loaders_with_windows_yield_what_all_yields(dev):
    a, w = small_exp('all'), small_exp('windows')
    la, lw = data.Gen1StoreLoader(a, 4, seed=2), data.Gen1StoreLoader(w, 4, seed=2)
    assert type(la.store) is data.Gen1Store and type(lw.store) is data.Gen1WindowStore and lw.store.capacity_bytes == lw.store.used_bytes
    assert lw.store.kept_records < lw.store.total_records == la.store.records.numel() // 8 and len(la) == len(lw) == 4
    assert data.gen1_store_for(w) is lw.store and data.gen1_store_for(w, 'test') is not lw.store
    n = 0
    for (fa, ta), (fw, tw) in zip(la, lw):
        assert torch.equal(fa, fw) and torch.equal(ta, tw) and fa.any() and fa.shape == (4, 1, TM, 2, *CANVAS)
        n += 1
    assert n == 4
    ids = [0, 5, 9, 2, 15, 7]
    ea, ew = data.Gen1StoreEvalLoader(a, 4, ids, data.gen1_store_for(a, 'test')), data.Gen1StoreEvalLoader(w, 4, ids, data.gen1_store_for(w, 'test'))
    assert type(ew.store) is data.Gen1WindowStore and type(ea.store) is data.Gen1Store
    for (fa, la_, (ha, wa), ia), (fw, lw_, (hw, ww), iw) in zip(ea, ew):
        assert torch.equal(fa, fw) and fa.any() and torch.equal(ia, iw) and torch.equal(ha, hw) and torch.equal(wa, ww)
        assert all(torch.equal(x, y) for x, y in zip(la_, lw_)) and len(la_) == len(lw_)


def test_experiment_hands_out_the_window_store_when_asked(dev):
    from yolox.exp import get_exp
    e = get_exp(None, 'e-yolox-s')
    e.train_input, e.store_recordings, e.store_records = 'dat_store', (2, 8, 3000), 'windows'
    e.merge(['input_size', '(64, 64)', 'test_size', '(64, 64)', 'num_classes', '2'])
    loader = e.get_data_loader(4, False)
    assert isinstance(loader, data.Gen1StoreLoader) and type(loader.store) is data.Gen1WindowStore and len(loader) == 4
    assert e.get_data_loader(4, False).store is loader.store
    ev = e.get_eval_loader(2, False)
    assert isinstance(ev, data.Gen1StoreEvalLoader) and type(ev.store) is data.Gen1WindowStore and ev.store is not loader.store
    e.store_records = 'most'
    with pytest.raises(ValueError):
        e.get_data_loader(4, False)


def test_frames_and_targets_replay_from_a_captured_graph(dev):
    exp = small_exp('windows')
    loader = data.Gen1StoreLoader(exp, 4, seed=5)
    store = loader.store
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
    idx.copy_(torch.from_numpy(i1))
    par.copy_(torch.from_numpy(p1))
    perm.copy_(torch.from_numpy(q1))
    frames.zero_()
    targets.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    eager_frames, eager_targets = chain()
    assert torch.equal(frames, eager_frames) and torch.equal(targets, eager_targets) and frames.any() and not np.array_equal(i0, i1)
    full = data.gen1_store_for(small_exp('all'))
    assert torch.equal(frames, full.frames(idx, par, exp)) and torch.equal(targets, full.targets(idx, par, perm, exp.input_size))


# ------------------------------------------------------------------------------------------------ the build
def test_build_from_a_directory_stays_inside_its_bound(dev, recordings, tmp_path):
    """the device holds the arena, one recording with the temporaries of its search and union, and the tables: at most ``capacity_bytes`` +
    2 x the largest recording + 1 MiB above what was allocated before; an arena that is too small raises and names the need"""
    for name, dat, rows in recordings:
        dat.tofile(str(tmp_path / f'{name}_td.dat'))
        np.save(str(tmp_path / f'{name}_bbox.npy'), rows)
    by_name = sorted(recordings, key=lambda r: r[0])                           # the order a directory is read in
    lay = ref.layout(by_name, 2)
    largest = max(len(dat) for _, dat, _ in recordings)
    capacity = 8 * lay['kept'] + 4096
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    win = data.Gen1WindowStore.from_directories(str(tmp_path), 2, ref.WINDOW, dev, capacity_bytes=capacity)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    print(f'peak {peak} bytes above the baseline; arena {capacity}, largest recording {largest}, all records {8 * lay["total"]}')
    assert peak <= capacity + 2 * largest + (1 << 20)
    assert win.kept_records == lay['kept'] and win.capacity_bytes == capacity and win.names == [r[0] for r in by_name]
    full = data.Gen1Store.from_directories(str(tmp_path), 2, ref.WINDOW, dev)
    idx = torch.arange(len(full), device=dev)
    par = [data.letterbox_params(*ref.SENSOR, *CANVAS)] * len(full)
    assert win.sample_names == full.sample_names and torch.equal(win.frames(idx, par, exp_for(2)), full.frames(idx, par, exp_for(2)))
    with pytest.raises(ValueError, match=str(8 * lay['kept'])):
        data.Gen1WindowStore.from_directories(str(tmp_path), 2, ref.WINDOW, dev, capacity_bytes=8 * lay['kept'] - 8)
    # no capacity given: the files' sizes bound the arena (far below the free memory here)
    auto = data.Gen1WindowStore.from_directories(str(tmp_path), 2, ref.WINDOW, dev)
    assert auto.kept_records == lay['kept'] and auto.capacity_bytes == sum(os.path.getsize(str(tmp_path / f'{r[0]}_td.dat')) for r in recordings) // 8 * 8
