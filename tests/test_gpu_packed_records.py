"""GPU tests of the Gen1 window store in packed records.  ``ops.records_pack`` / ``ops.records_unpack`` against the numpy checker
(tests/packed_records_ref.py), byte for byte, with canary bytes around the units of a call; the packed-range frame operators against the
existing ``ops.event_histogram_dat_ranges`` / ``ops.event_latest_surface_dat_ranges`` on the records that were packed;
``data.Gen1PackedWindowStore`` against ``data.Gen1WindowStore`` on the same recordings -- frames, targets, records, loaders, a captured
graph, two ranks -- and the memory its build takes.  Everything is a copy, index work or integer binning: every comparison is exact."""
import gc
import types

import numpy as np
import pytest
import torch

import packed_records_ref as ref
import window_store_ref
from eas_snn_amd import _lib, data, ops

pytestmark = pytest.mark.gpu

SENSORS = [(240, 304), (12, 20), (12, 16), (12, 17)]
COUNTS = [1, 63, 64, 65, 64 * 1024 + 1]
CANARY = 0xA5
CANVAS, TM = (64, 96), 4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    return torch.device('cuda:0')


def on(dev, rec):
    return torch.from_numpy(ref.as_bytes(rec)).to(dev)


def bits(table):
    return table.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ pack and unpack
def run_pack(dev, rec, H, W, unit_offset=0, tail_units=2):
    """the op and the checker on the same records: the table and the whole arena, canary units in front of and behind the call's units
    included, must agree"""
    want_table, want_payload = ref.pack(rec, H, W, unit_offset)
    arena = np.full(ref.UNIT * (unit_offset + tail_units) + len(want_payload), CANARY, dtype=np.uint8)
    want = arena.copy()
    want[ref.UNIT * unit_offset:ref.UNIT * unit_offset + len(want_payload)] = want_payload
    d = torch.from_numpy(arena).to(dev)
    table = torch.full((len(want_table), 2), -1, dtype=torch.int32, device=dev)
    units = ops.records_pack(on(dev, rec), table, d, unit_offset, H, W)
    assert units * ref.UNIT == len(want_payload)
    assert np.array_equal(bits(table), want_table)
    assert np.array_equal(d.cpu().numpy(), want)
    return table, d, want_table


@pytest.mark.parametrize('H,W', SENSORS)
def test_pack_equals_the_checker_byte_for_byte(dev, H, W):
    """1, 63, 64, 65 and 64 k + 1 records holding blocks of every kind (ref.KINDS: the longest narrow span and one microsecond more, the
    largest narrow x and y and one more, bit 29, time stepping backwards, equal times, events outside the sensor); behind unit 0 and unit 3"""
    for n in COUNTS:
        rec, kinds = ref.records_of_every_kind(H, W, n, seed=n)
        for unit_offset in (0, 3):
            _, _, table = run_pack(dev, rec, H, W, unit_offset)
        whole = n // 64
        assert np.array_equal((table[:, 1] >> 31).astype(bool)[:whole], ref.expected_wide(kinds, H, W)[:whole])
    assert whole > len(ref.KINDS) and (table[:, 1] >> 31).any() and not (table[:, 1] >> 31).all()


def test_dry_run_fills_the_table_and_leaves_the_arena(dev):
    H, W = 240, 304
    rec, _ = ref.records_of_every_kind(H, W, 64 * 11 + 9)
    want_table, want_payload = ref.pack(rec, H, W, 7)
    arena = torch.full((64,), CANARY, dtype=torch.uint8, device=dev)                          # far too small: never looked at
    table = torch.full((12, 2), -1, dtype=torch.int32, device=dev)
    assert ops.records_pack(on(dev, rec), table, arena, 7, H, W, dry_run=True) * ref.UNIT == len(want_payload)
    assert np.array_equal(bits(table), want_table) and (arena == CANARY).all()


def test_an_arena_one_unit_too_small_raises_and_stays_untouched(dev):
    H, W = 240, 304
    rec, _ = ref.records_of_every_kind(H, W, 64 * 11 + 9)
    units = len(ref.pack(rec, H, W)[1]) // ref.UNIT
    for unit_offset in (0, 2):
        arena = torch.full((ref.UNIT * (unit_offset + units - 1),), CANARY, dtype=torch.uint8, device=dev)
        table = torch.empty((12, 2), dtype=torch.int32, device=dev)
        with pytest.raises(ops.PackedArenaFull, match=str(ref.UNIT * (unit_offset + units))) as err:
            ops.records_pack(on(dev, rec), table, arena, unit_offset, H, W)
        assert err.value.units == units and isinstance(err.value, ValueError) and (arena == CANARY).all()
        exact = torch.full((ref.UNIT * (unit_offset + units),), CANARY, dtype=torch.uint8, device=dev)
        assert ops.records_pack(on(dev, rec), table, exact, unit_offset, H, W) == units


@pytest.mark.parametrize('H,W', [(240, 304), (12, 17)])
def test_unpack_gives_the_records_back(dev, H, W):
    """whole, and sub-ranges that begin and end in the middle of narrow and of wide blocks (ref.KINDS: block 1 is narrow, block 2 wide)"""
    n = 64 * 13 + 20
    rec, kinds = ref.records_of_every_kind(H, W, n, seed=4)
    wide = ref.expected_wide(kinds, H, W)
    assert not wide[1] and wide[2] and not wide[3] and wide[4] and wide[5]
    table, arena, want_table = run_pack(dev, rec, H, W, 3)
    _, payload = ref.pack(rec, H, W, 3)
    nb = len(want_table)
    for a, e in ((0, n), (64 + 17, 2 * 64 + 40), (2 * 64 + 5, 2 * 64 + 50), (2 * 64 + 63, 3 * 64 + 1), (4 * 64 + 9, 6 * 64 - 9), (3 * 64 + 1, 3 * 64 + 2),
                 (70, 70), (n - 3, nb * 64), (0, 0), (nb * 64, nb * 64)):
        got, flags = ops.records_unpack(table, arena, a, e, H, W, return_flags=True)
        got = got.cpu().numpy().view(np.uint32).reshape(-1, 2)
        assert np.array_equal(got, ref.unpack(want_table, payload, a, e, H, W, unit_offset=3)), (a, e)
        assert np.array_equal(got[:max(min(e, n) - a, 0)], rec[a:min(e, n)]) and int(flags) == 0
        assert (got[max(n - a, 0):] == rec[-1]).all()                                          # the padding: copies of the last record
    for a, e in ((-1, 5), (5, 4), (0, nb * 64 + 1)):
        with pytest.raises(ValueError):
            ops.records_unpack(table, arena, a, e, H, W)


# ------------------------------------------------------------------------------------------------ frames
def frame_ranges(n, nb):
    """unsorted, overlapping, empty, of one record, beginning and ending mid-block, spanning narrow and wide blocks (blocks 2, 4, 5, 8 are
    wide), the whole store, the last records"""
    return np.array([(5 * 64 + 3, 9 * 64 + 60), (0, n), (64 + 17, 2 * 64 + 40), (100, 100), (2 * 64 + 5, 2 * 64 + 50), (3 * 64 + 1, 3 * 64 + 2),
                     (64, 4 * 64), (0, 64), (6 * 64, 7 * 64), (n - 200, n), (0, 0), (n, n), (6 * 64 + 20, 7 * 64 + 31), (9 * 64 + 1, 20 * 64 - 5)],
                    dtype=np.int64)


@pytest.mark.parametrize('H,W', [(240, 304), (12, 17), (12, 16)])
@pytest.mark.parametrize('Tm', [1, 4, 5])
def test_frames_equal_the_dat_range_operators(dev, H, W, Tm):
    n = 64 * 22 + 30
    rec, _ = ref.records_of_every_kind(H, W, n, seed=9)
    records = on(dev, rec)
    nb = (n + 63) // 64
    table = torch.empty((nb, 2), dtype=torch.int32, device=dev)
    arena = torch.empty(ref.UNIT * 2 * nb, dtype=torch.uint8, device=dev)
    units = ops.records_pack(records, table, arena, 0, H, W)
    payload = arena[:ref.UNIT * units]
    ranges = torch.from_numpy(frame_ranges(n, nb)).to(dev)
    want, want_oob = ops.event_histogram_dat_ranges(records, ranges, Tm, H, W, return_oob=True)
    got, oob, flags = ops.event_histogram_packed_ranges(table, payload, ranges, Tm, H, W, return_oob=True, return_flags=True)
    assert got.dtype == torch.int32 and got.shape == (len(ranges), Tm, 2, H, W) and torch.equal(got, want)
    assert int(oob) == int(want_oob) > 0 and int(flags) == 0 and int(want.sum()) > 0
    assert torch.equal(ops.event_histogram_packed_ranges(table, payload, ranges, Tm, H, W), want)
    want, want_oob = ops.event_latest_surface_dat_ranges(records, ranges, Tm, H, W, tau=3e4, return_oob=True)
    got, oob, flags = ops.event_latest_surface_packed_ranges(table, payload, ranges, Tm, H, W, tau=3e4, return_oob=True, return_flags=True)
    assert got.dtype == torch.float64 and torch.equal(got.view(torch.int64), want.view(torch.int64))
    assert int(oob) == int(want_oob) > 0 and int(flags) == 0 and bool(want.any())
    one = ranges[2:3]                                                                          # a batch of one, default tau
    assert torch.equal(ops.event_latest_surface_packed_ranges(table, payload, one, Tm, H, W),
                       ops.event_latest_surface_dat_ranges(records, one, Tm, H, W))


def test_what_arrives_as_device_data_is_bounded(dev):
    """a range outside the packed records is walked as empty and flagged (bit 0); a table entry that places a block outside the payload is
    skipped and flagged (bit 1).  Both rely on the bound the operators state: nothing outside the table and the payload is addressed."""
    H, W, Tm = 240, 304, 4
    n = 64 * 12
    rec, _ = ref.records_of_every_kind(H, W, n, seed=2)
    records = on(dev, rec)
    table = torch.empty((12, 2), dtype=torch.int32, device=dev)
    arena = torch.empty(ref.UNIT * 24, dtype=torch.uint8, device=dev)
    units = ops.records_pack(records, table, arena, 0, H, W)
    payload = arena[:ref.UNIT * units]
    ranges = torch.tensor([[-1, 10], [5, n + 1], [10, 5], [0, 50], [-(1 << 40), 1 << 40]], dtype=torch.int64, device=dev)
    ok = torch.tensor([[0, 0], [0, 0], [0, 0], [0, 50], [0, 0]], dtype=torch.int64, device=dev)
    for op, ref_op in ((ops.event_histogram_packed_ranges, ops.event_histogram_dat_ranges),
                       (ops.event_latest_surface_packed_ranges, ops.event_latest_surface_dat_ranges)):
        got, flags = op(table, payload, ranges, Tm, H, W, return_flags=True)
        assert int(flags) == ops.RECORDS_FLAG_RANGE and torch.equal(got, ref_op(records, ok, Tm, H, W)) and bool(got[3].any())
        assert not got[[0, 1, 2, 4]].any()
        flags.fill_(-1)
        assert int(op(table, payload, ok, Tm, H, W, return_flags=True)[1]) == 0                # written, not accumulated
    # the payload cut short by the last block's units: its records are skipped, the blocks in front read as before
    last = int(bits(table)[-1, 1] & 0x7fffffff)
    short = payload[:ref.UNIT * last]
    ranges = torch.tensor([[0, 11 * 64], [11 * 64, 12 * 64], [10 * 64, 12 * 64], [3, 200]], dtype=torch.int64, device=dev)
    got, flags = ops.event_histogram_packed_ranges(table, short, ranges, Tm, H, W, return_flags=True)
    want = ops.event_histogram_dat_ranges(records, ranges, Tm, H, W)
    assert int(flags) == ops.RECORDS_FLAG_TABLE and torch.equal(got[[0, 3]], want[[0, 3]]) and not got[[1, 2]].any()
    out, flags = ops.records_unpack(table, short, 10 * 64, 12 * 64, H, W, return_flags=True)
    out = out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert int(flags) == ops.RECORDS_FLAG_TABLE and np.array_equal(out[:64], rec[10 * 64:11 * 64]) and not out[64:].any()


# ------------------------------------------------------------------------------------------------ the store
@pytest.fixture(scope='module')
def recordings():
    return window_store_ref.recordings()


@pytest.fixture(scope='module')
def stores(dev, recordings):
    """{Tl: (the window store -- the oracle, pinned to the full store by its own tests --, the packed store)}"""
    W = window_store_ref.WINDOW
    return {Tl: (data.Gen1WindowStore(recordings, Tl, W, dev), data.Gen1PackedWindowStore(recordings, Tl, W, dev)) for Tl in (1, 2)}


def exp_for(Tl, aggregation='micro_sum', **kw):
    return types.SimpleNamespace(Tm=TM, Tl=Tl, input_size=CANVAS, test_size=CANVAS, num_classes=2, window=-20, aggregation=aggregation, **kw)


def checker_layout(win):
    """what the checker packs of the window store's records, every recording on a fresh block: (table, payload, first logical record of
    every recording)"""
    rows = win.records.cpu().numpy().view(np.uint32).reshape(-1, 2)
    tables, parts, unit, first = [], [], 0, [0]
    for a, e in zip(win.host['file_offsets'][:-1], win.host['file_offsets'][1:]):
        t, p = ref.pack(rows[a:e], *window_store_ref.SENSOR, unit_offset=unit)
        tables.append(t)
        parts.append(p)
        unit += len(p) // ref.UNIT
        first.append(first[-1] + 64 * len(t))
    return np.concatenate(tables), np.concatenate(parts), np.asarray(first, dtype=np.int64)


@pytest.mark.parametrize('Tl,narrow,wide', [(1, 1509, 22), (2, 3041, 4)])
def test_store_holds_what_the_checker_packs(dev, stores, Tl, narrow, wide):
    win, packed = stores[Tl]
    table, payload, first = checker_layout(win)
    assert packed.narrow_blocks == narrow and packed.wide_blocks == wide            # a condition on the inputs: blocks of both kinds
    assert np.array_equal(bits(packed.table), table) and np.array_equal(packed.payload.cpu().numpy(), payload)
    assert packed.records is None and packed.kept_records == win.kept_records and packed.total_records == win.total_records
    assert packed.used_bytes == len(payload) == packed.payload.numel() and packed.capacity_bytes >= packed.used_bytes
    blocks = narrow + wide
    assert packed.nbytes() == len(payload) + 8 * blocks == 264 * narrow + 520 * wide
    assert packed.nbytes() <= 8 * 64 * blocks + 8 * blocks and packed.nbytes() <= 8 * win.kept_records + (512 + 8) * len(win.names) + 8 * blocks
    assert packed.nbytes() < 0.54 * win.used_bytes
    assert packed.file_offsets.tolist() == first.tolist()
    # every sample range: the same records, at logical indices that skip the padding
    pr, wr = packed.sample_ranges.cpu().numpy(), win.sample_ranges.cpu().numpy()
    assert pr.shape == wr.shape == (30, Tl, 2) and np.array_equal(pr[..., 1] - pr[..., 0], wr[..., 1] - wr[..., 0])
    rows = win.records.view(torch.int64)
    for (a, e), (pa, pe) in zip(wr.reshape(-1, 2), pr.reshape(-1, 2)):
        assert torch.equal(packed.unpacked(int(pa), int(pe)).view(torch.int64), rows[a:e])
    # the parent's tables, names and labels
    assert packed.sample_names == win.sample_names and packed.names == win.names and packed.max_group_rows == win.max_group_rows
    for k in ('boxes', 'group_start', 'group_t', 'group_file'):
        assert torch.equal(getattr(packed, k), getattr(win, k))
    assert np.array_equal(packed.raw_labels(11), win.raw_labels(11))


@pytest.mark.parametrize('aggregation', ['micro_sum', 'timesurface'])
@pytest.mark.parametrize('Tl', [1, 2])
def test_store_frames_and_targets_equal_the_window_store(dev, stores, Tl, aggregation):
    win, packed = stores[Tl]
    exp = exp_for(Tl, aggregation)
    rs = np.random.RandomState(5)
    idx = torch.from_numpy(rs.permutation(len(win)).astype(np.int64)).to(dev)
    par = np.array([data.jitter_params(*window_store_ref.SENSOR, *CANVAS, jitter=.3, rng=rs) for _ in range(len(win))], dtype=np.int32)
    assert set(par[:, 4]) == {0, 1}                                             # flipped and not
    par = torch.from_numpy(par).to(dev)
    want, got = win.frames(idx, par, exp), packed.frames(idx, par, exp)
    assert got.shape == (30, Tl, TM, 2, *CANVAS) and got.dtype == torch.float32 and torch.equal(got, want)
    assert want.reshape(30, -1).any(1).sum() == 27                              # all but the gap label and 'noevents'
    assert torch.equal(packed.targets(idx, par, None, CANVAS), win.targets(idx, par, None, CANVAS))
    for b in (0, 7, 29):                                                        # every sample alone, too (a batch of one)
        assert torch.equal(packed.frames(idx[b:b + 1], par[b:b + 1], exp), want[b:b + 1])
    with pytest.raises(ValueError):
        packed.frames(idx, par, exp_for(3 - Tl, aggregation))


def test_trim_keeps_the_frames(dev, recordings):
    win, exp = data.Gen1WindowStore(recordings[:2], 1, window_store_ref.WINDOW, dev), exp_for(1)
    packed = data.Gen1PackedWindowStore(recordings[:2], 1, window_store_ref.WINDOW, dev, capacity_bytes=4_000_000)
    idx = torch.arange(len(win), device=dev)
    par = [data.letterbox_params(*window_store_ref.SENSOR, *CANVAS)] * len(win)
    assert packed.capacity_bytes == 4_000_000 // 256 * 256 > packed.used_bytes and packed.trim() is packed
    assert packed.capacity_bytes == packed.used_bytes == packed.payload.untyped_storage().nbytes()
    assert packed.table.untyped_storage().nbytes() == 8 * (packed.narrow_blocks + packed.wide_blocks)
    assert torch.equal(packed.frames(idx, par, exp), win.frames(idx, par, exp))


def test_two_ranks_hold_the_store_between_them(dev, stores, recordings):
    win, whole = stores[1]
    exp = exp_for(1)
    halves = [data.Gen1PackedWindowStore(recordings, 1, window_store_ref.WINDOW, dev, shard=(r, 2)) for r in (0, 1)]
    assert sum(h.kept_records for h in halves) == whole.kept_records and sum(h.total_records for h in halves) == whole.total_records
    assert sum(h.narrow_blocks for h in halves) == whole.narrow_blocks and sum(h.wide_blocks for h in halves) == whole.wide_blocks
    assert sorted(np.concatenate([h.owned_samples for h in halves]).tolist()) == list(range(len(whole)))
    par = torch.from_numpy(np.array([data.letterbox_params(*window_store_ref.SENSOR, *CANVAS)] * len(whole), dtype=np.int32)).to(dev)
    for r, h in enumerate(halves):
        assert h.shard == (r, 2) and h.sample_ranges.shape == whole.sample_ranges.shape and len(h.owned_samples) > 0
        own = torch.from_numpy(h.owned_samples).to(dev)
        assert torch.equal(h.frames(own, par[own], exp), win.frames(own, par[own], exp))
        assert torch.equal(h.targets(own, par[own], None, CANVAS), win.targets(own, par[own], None, CANVAS))
        with pytest.raises(IndexError):
            h.check_owned(halves[1 - r].owned_samples[:1])


# ------------------------------------------------------------------------------------------------ loaders and capture
def small_exp(store_events):
    return exp_for(1, store_records='windows', store_events=store_events, store_recordings=(2, 8, 3000))


def test_one_epoch_through_the_selection_yields_the_window_stores_batches(dev):
    w, p = small_exp('dat'), small_exp('packed')
    lw, lp = data.Gen1StoreLoader(w, 4, seed=2), data.Gen1StoreLoader(p, 4, seed=2)
    assert type(lw.store) is data.Gen1WindowStore and type(lp.store) is data.Gen1PackedWindowStore
    assert lp.store.capacity_bytes == lp.store.used_bytes and lp.store.kept_records == lw.store.kept_records and len(lw) == len(lp) == 4
    assert data.gen1_store_for(p) is lp.store and data.gen1_store_for(p, 'test') is not lp.store
    p.store_events = 'dat'
    assert type(data.gen1_store_for(p)) is data.Gen1WindowStore                   # a cache of their own: the other kind is not handed out
    p.store_events = 'packed'
    n = 0
    for (fw, tw), (fp, tp) in zip(lw, lp):
        assert torch.equal(fw, fp) and torch.equal(tw, tp) and fw.any() and fw.shape == (4, 1, TM, 2, *CANVAS)
        n += 1
    assert n == 4
    ids = [0, 5, 9, 2, 15, 7]
    ew, ep = data.Gen1StoreEvalLoader(w, 4, ids, data.gen1_store_for(w, 'test')), data.Gen1StoreEvalLoader(p, 4, ids, data.gen1_store_for(p, 'test'))
    assert type(ep.store) is data.Gen1PackedWindowStore
    for (fw, lw_, (hw, ww), iw), (fp, lp_, (hp, wp), ip) in zip(ew, ep):
        assert torch.equal(fw, fp) and fw.any() and torch.equal(iw, ip) and torch.equal(hw, hp) and torch.equal(ww, wp)
        assert all(torch.equal(x, y) for x, y in zip(lw_, lp_)) and len(lw_) == len(lp_)
    with pytest.raises(ValueError, match='store_events'):
        data.gen1_store_for(exp_for(1, store_records='all', store_events='packed', store_recordings=(2, 8, 3000)))


def test_frames_and_targets_replay_from_a_captured_graph(dev):
    exp = small_exp('packed')
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
    win = data.gen1_store_for(small_exp('dat'))
    assert torch.equal(frames, win.frames(idx, par, exp)) and torch.equal(targets, win.targets(idx, par, perm, exp.input_size))


# ------------------------------------------------------------------------------------------------ the build
def test_build_from_a_directory_stays_inside_its_bound(dev, recordings, tmp_path):
    """the device holds the arena, the table (8 bytes per unit of the arena), one recording with the temporaries of its search and union,
    that recording's kept records, and the tables: at most ``capacity_bytes`` + ``capacity_bytes`` / 32 + 2 x the largest recording + the
    most records kept of one recording + 1 MiB above what was allocated before; an arena that is too small raises and names the need"""
    for name, dat, rows in recordings:
        dat.tofile(str(tmp_path / f'{name}_td.dat'))
        np.save(str(tmp_path / f'{name}_bbox.npy'), rows)
    by_name = sorted(recordings, key=lambda r: r[0])                           # the order a directory is read in
    win = data.Gen1WindowStore(by_name, 2, window_store_ref.WINDOW, dev)
    need = len(checker_layout(win)[1])
    largest = max(len(dat) for _, dat, _ in recordings)
    largest_kept = 8 * int(np.diff(win.host['file_offsets']).max())
    capacity = need + 4096
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    packed = data.Gen1PackedWindowStore.from_directories(str(tmp_path), 2, window_store_ref.WINDOW, dev, capacity_bytes=capacity)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    print(f'peak {peak} bytes above the baseline; arena {capacity}, largest recording {largest}, its kept records {largest_kept}')
    assert peak <= capacity + capacity // 32 + 2 * largest + largest_kept + (1 << 20)
    assert packed.kept_records == win.kept_records and packed.capacity_bytes == capacity and packed.names == [r[0] for r in by_name]
    assert packed.used_bytes == need
    idx = torch.arange(len(win), device=dev)
    par = [data.letterbox_params(*window_store_ref.SENSOR, *CANVAS)] * len(win)
    assert packed.sample_names == win.sample_names and torch.equal(packed.frames(idx, par, exp_for(2)), win.frames(idx, par, exp_for(2)))
    with pytest.raises(ValueError, match=str(need)):
        data.Gen1PackedWindowStore.from_directories(str(tmp_path), 2, window_store_ref.WINDOW, dev, capacity_bytes=need - 256)
    exact = data.Gen1PackedWindowStore.from_directories(str(tmp_path), 2, window_store_ref.WINDOW, dev, capacity_bytes=need)
    assert exact.used_bytes == exact.capacity_bytes == need
