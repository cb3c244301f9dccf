"""GPU tests of the 1 Mpx store in packed rows.  ``ops.count_rows_pack`` against the numpy statement of the format
(tests/packed_store_ref.py) bit for bit, in one piece and in two chunks behind a non-zero unit, with every byte of the arena outside the used
range left as it was; ``ops.count_rows_unpack`` back to the sums; ``ops.packed_store_frames`` against ``ops.count_store_frames`` on the
same sums, frames and flags, at the shapes where the row kernels and the band kernel can go wrong; ``data.Gen4PackedStore`` against
``data.Gen4Store`` and tests/golden/gen4_store.npz; the loaders, a short Trainer run and a captured graph with ``exp.store_sums =
'packed'``.  Every value is an integer or the result of the one arithmetic both sides share, so every comparison is exact.

Sensors (H x W): 6 x 16 one group; 5 x 40 ``W % 8 == 0`` with a half-full last group; 4 x 37 rows that are not 16-byte aligned; 2 x 1024
64 groups, bit 63 of the masks and ``below(63)``.  Contents (``packed_store_ref.fields``): zeros; every pixel 255; one pixel 256; one pixel
65 025 in the last column; groups alternating zero / narrow / wide; seeded sparse fields at densities 0.02 and 0.3 with values up to 300.
A band of fewer than eight rows exists inside ``W <= 1024``: the 1024-pixel sensor on a 2064-pixel canvas (``frames_band_rows``: 4 rows)."""
import functools
import gc
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

import gen4_store_ref
import packed_store_ref as ref
from eas_snn_amd import _lib, data, ops
from test_gpu_hist_store import BASE_OPTS, dev  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(6, 16), (5, 40), (4, 37), (2, 1024)]
IDS = ['one_group', 'w40_half_group', 'w37_elements', 'w1024_64_groups']
FILL = 0xA5


@functools.lru_cache(maxsize=None)
def case(H, W):
    """(sums u16 [7, 2, H, W], the checker's table, the checker's payload) -- computed once, never written"""
    f = ref.fields(H, W)
    table, payload = ref.encode(f)
    for a in (f, table, payload):
        a.setflags(write=False)
    return f, table, payload


def up(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def i64(v, dev):
    return torch.tensor(list(v), dtype=torch.int64, device=dev)


def same16(a, b):
    """``torch.equal`` of two uint16 tensors (compared as the int16 they alias)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------ pack and unpack
@pytest.mark.parametrize('H,W', SHAPES, ids=IDS)
def test_pack_equals_the_checker(dev, H, W):
    f, table, payload = case(H, W)
    sums, n = up(f, dev), len(payload)
    arena = torch.full((n + 64,), FILL, dtype=torch.uint8, device=dev)
    tab = torch.full((7, 2, H, 3), -1, dtype=torch.int64, device=dev)
    used = ops.count_rows_pack(sums, tab, arena, 0)
    got = arena.cpu().numpy()
    assert used * 16 == n and np.array_equal(tab.cpu().numpy(), table)
    assert np.array_equal(got[:n], payload) and (got[n:] == FILL).all()
    # in two chunks behind unit 3: the rows of a chunk follow the position reached; the front, the seam and the rest stay as they were
    arena = torch.full((48 + n + 48,), FILL, dtype=torch.uint8, device=dev)
    tab = torch.full((7, 2, H, 3), -1, dtype=torch.int64, device=dev)
    u1 = ops.count_rows_pack(sums[:3], tab[:3], arena, 3)
    mid = arena.cpu().numpy()
    assert (mid[:48] == FILL).all() and (mid[48 + 16 * u1:] == FILL).all()
    u2 = ops.count_rows_pack(sums[3:], tab[3:], arena, 3 + u1)
    want = table.copy()
    want[..., 2] += 3
    got = arena.cpu().numpy()
    assert (u1 + u2) * 16 == n and np.array_equal(tab.cpu().numpy(), want)
    assert (got[:48] == FILL).all() and np.array_equal(got[48:48 + n], payload) and (got[48 + n:] == FILL).all()
    # an arena one unit too small: ValueError that names the bytes needed, nothing written; a dry run fills the table only
    small = torch.full((n - 16,), FILL, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match=str(n)) as err:
        ops.count_rows_pack(sums, tab, small, 0)
    assert err.value.units * 16 == n and (small == FILL).all().item()
    tab.fill_(-1)
    assert ops.count_rows_pack(sums, tab, small, 0, dry_run=True) * 16 == n and (small == FILL).all().item()
    assert np.array_equal(tab.cpu().numpy(), table)
    # n = 0: no launch, nothing read back
    assert ops.count_rows_pack(sums[:0], tab[:0], small, 0) == 0


@pytest.mark.parametrize('H,W', SHAPES, ids=IDS)
def test_unpack_returns_the_sums(dev, H, W):
    f, table, payload = case(H, W)
    tab, pay = up(table, dev), up(payload, dev)
    got = ops.count_rows_unpack(tab, pay, W)
    assert got.dtype == torch.uint16 and got.shape == (7, 2, H, W) and np.array_equal(got.cpu().numpy(), f)
    assert np.array_equal(ops.count_rows_unpack(tab[2:6], pay, W).cpu().numpy(), f[2:6])          # a range: the offsets stay whole-payload positions
    assert ops.count_rows_unpack(tab[3:3], pay, W).shape == (0, 2, H, W)
    # what the device packed, behind a non-zero unit
    arena = torch.zeros(16 * 5 + len(payload), dtype=torch.uint8, device=dev)
    mine = torch.empty_like(tab)
    used = ops.count_rows_pack(up(f, dev), mine, arena, 5)
    assert np.array_equal(ops.count_rows_unpack(mine, arena[:16 * (5 + used)], W).cpu().numpy(), f)
    # a table that points behind the payload is not followed: those groups come out as zeros
    cut = ops.count_rows_unpack(tab, pay[:len(payload) // 32 * 16], W).cpu().numpy()
    assert np.array_equal(cut[0], f[0]) and not np.array_equal(cut, f) and ((cut == f) | (cut == 0)).all()


# ------------------------------------------------------------------------------------------------ frames
def both(dev, sums, first, Tm, Hc, Wc, lo=None, params=None):
    """``packed_store_frames`` on the packed form of ``sums`` (a device tensor); asserts that frames and flags equal ``count_store_frames`` on
    ``sums`` itself; returns (frames, flags)"""
    R, _, H, W = sums.shape
    tab = torch.empty((R, 2, H, 3), dtype=torch.int64, device=dev)
    arena = torch.empty(R * 2 * H * ((W + 15) // 16) * 32, dtype=torch.uint8, device=dev)
    used = ops.count_rows_pack(sums, tab, arena, 0)
    kw = dict(lo=None if lo is None else i64(lo, dev), params=None if params is None else torch.tensor(params, dtype=torch.int32, device=dev),
              return_flags=True)
    out, flags = ops.packed_store_frames(tab, arena[:16 * used], i64(first, dev), Tm, Hc, Wc, W=W, **kw)
    want, want_flags = ops.count_store_frames(sums, i64(first, dev), Tm, Hc, Wc, **kw)
    assert out.shape == (len(first), 1, Tm, 2, Hc, Wc) and out.dtype == torch.float32 and flags.shape == (len(first),) and flags.dtype == torch.int32
    assert torch.equal(out, want) and torch.equal(flags, want_flags)
    return out, flags


def jittered(H, W, Hc, Wc, B, flip, seed):
    rs = np.random.RandomState(seed)
    return [data.jitter_params(H, W, Hc, Wc, jitter=.3, rng=rs)[:4] + (flip,) for _ in range(B)]


@pytest.mark.parametrize('H,W', SHAPES, ids=IDS)
def test_frames_equal_the_u16_store(dev, H, W):
    """R = 7; samples: two zero slices in front, a neighbour recording in front (``first`` below ``lo``), plain, the end of the store
    (flag bit), a copy in the middle"""
    sums = up(case(H, W)[0], dev)
    first, lo = [-2, 3, 4, 5, 1], [0, 4, 4, 4, 0]
    for Hc, Wc in ((32, 64), (64, 64), (3, 16)):                    # (the last: smaller than every sensor but the 6 x 16 one's width)
        for Tm in (1, 3):
            for k, params in enumerate((None, jittered(H, W, Hc, Wc, 5, 0, Tm), jittered(H, W, Hc, Wc, 5, 1, 7 + Tm),
                                        [(W, H, 0, 0, 0), (W, H, 3, 1, 1), (max(W // 2, 1), 2 * H, 2, 0, 1), (W + 7, max(H - 1, 1), -3, 1, 0),
                                         (0, H, 1, 1, 0)])):
                out, flags = both(dev, sums, first, Tm, Hc, Wc, lo=lo, params=params)
                assert flags.tolist() == [0, 0, 0, int(5 + Tm > 7), 0], (Hc, Wc, Tm, k)
                if params is None:
                    assert out[4].any().item() and not out[0, 0, :Tm - 1].any().item()
                    assert np.array_equal(out[2, 0, 0, :, :min(H, Hc), :min(W, Wc)].cpu().numpy(), case(H, W)[0][4, :, :min(H, Hc), :min(W, Wc)])
    out, flags = both(dev, sums, [-2, 6, -10 ** 15, 10 ** 15, 2 ** 63 - 1, -2 ** 63], 3, 32, 64)
    assert flags.tolist() == [0, 1, 0, 1, 1, 0] and not out[2:].any().item()


def test_frames_bands_shorter_than_eight_rows(dev):
    """the 1024-pixel sensor on a canvas of 2064 columns: bands of 4 rows (``frames_band_rows``), three bands on 11 canvas rows"""
    assert 2 * 8 * 1024 * 2 + 2064 * 8 > 48 * 1024 >= 2 * 4 * 1024 * 2 + 2064 * 8
    sums = up(case(2, 1024)[0], dev)
    for rows in (None, [(900, 7, 100, 2, 1), (1024, 2, 0, 0, 0)], [(2000, 9, 30, 1, 0), (640, 5, -300, -2, 1)]):
        out, flags = both(dev, sums, [4, 5], 2, 11, 2064, params=rows)
        assert out[0].any().item() and out[1].any().item() and not flags.any().item(), rows


# ------------------------------------------------------------------------------------------------ the store
def synth(nbins):
    """2 files x 6 representations on a 24 x 48 sensor; two pixels of the first file made wide (every bin at 255)"""
    recs = data.synth_gen4_recordings(2, 6, (24, 48), nbins, 3, seed=3)
    recs[0][1][1, :nbins, 3, 5] = 255
    recs[0][1][4, nbins:, 23, 47] = 255
    return recs


def small_exp(**kw):
    return types.SimpleNamespace(Tm=3, Tl=1, input_size=(32, 64), test_size=(32, 64), num_classes=3, **kw)


@pytest.mark.parametrize('nbins', [10, 3])
def test_store_equals_the_parent(dev, nbins):
    recs = synth(nbins)
    parent = data.Gen4Store(recs, 3, dev, sensor_hw=(24, 48), nbins=nbins, chunk=4)
    a = data.Gen4PackedStore(recs, 3, dev, sensor_hw=(24, 48), nbins=nbins, chunk=4)
    b = data.Gen4PackedStore(recs, 3, dev, sensor_hw=(24, 48), nbins=nbins, chunk=64)
    table, payload = ref.encode(parent.sums.cpu().numpy())
    assert parent.sums.cpu().numpy().max() == 255 * nbins
    for s in (a, b):
        assert s.sums is None and s.rows.shape == (12, 2, 24, 3) and s.rows.dtype == torch.int64 and s.payload.dtype == torch.uint8
        assert np.array_equal(s.rows.cpu().numpy(), table) and np.array_equal(s.payload.cpu().numpy(), payload)
        assert s.used_bytes == len(payload) == s.payload.numel() and s.nbytes == len(payload) + table.nbytes
        assert s.capacity_bytes == parent.sums.numel() * 2                                  # W % 16 == 0: the u16 size
        assert same16(s.unpacked(0, 12), parent.sums) and same16(s.unpacked(5, 9), parent.sums[5:9])
    assert a.nbytes < parent.sums.numel() * 2
    exp = small_exp()
    idx = torch.arange(len(parent), device=dev)
    assert len(a) == len(parent) == 6 and a.sample_names == parent.sample_names
    rs = np.random.RandomState(1)
    par = np.array([data.jitter_params(24, 48, 32, 64, jitter=.3, rng=rs) for _ in range(6)], dtype=np.int32)
    perm = torch.from_numpy(np.stack([rs.permutation(3) for _ in range(6)]).astype(np.int32)).to(dev)
    for params in (None, par):
        want = parent.frames(idx, params, exp)
        assert torch.equal(a.frames(idx, params, exp), want) and want.any().item()
    assert torch.equal(a.frames(idx, par, exp, canvas_hw=(64, 64)), parent.frames(idx, par, exp, canvas_hw=(64, 64)))
    assert torch.equal(a.targets(idx, par, perm, (32, 64)), parent.targets(idx, par, perm, (32, 64)))
    assert all(np.array_equal(a.raw_labels(i), parent.raw_labels(i)) for i in range(6))
    # the shards of a world of 2
    for r in (0, 1):
        half, want = (cls(recs, 3, dev, sensor_hw=(24, 48), nbins=nbins, chunk=4, shard=(r, 2)) for cls in (data.Gen4PackedStore, data.Gen4Store))
        assert half.shard == (r, 2) and np.array_equal(half.owned_samples, want.owned_samples) and len(half.owned_samples) == 3
        assert same16(half.unpacked(0, 6), want.sums) and half.rows.shape[0] == 6 and torch.equal(half.held_first, want.held_first)
        assert torch.equal(half.frames(idx, par, exp), want.frames(idx, par, exp))
        mine = torch.from_numpy(half.owned_samples).to(dev)
        assert torch.equal(half.frames(mine, par[half.owned_samples], exp), parent.frames(mine, par[half.owned_samples], exp))
    # capacity: one unit too small raises and names the need; trim gives the rest back
    with pytest.raises(ValueError, match=str(len(payload))):
        data.Gen4PackedStore(recs, 3, dev, sensor_hw=(24, 48), nbins=nbins, chunk=4, capacity_bytes=len(payload) - 16)
    exact = data.Gen4PackedStore(recs, 3, dev, sensor_hw=(24, 48), nbins=nbins, chunk=4, capacity_bytes=len(payload))
    assert exact.used_bytes == exact.capacity_bytes == len(payload)
    want = a.frames(idx, par, exp)
    assert a.capacity_bytes > a.used_bytes and a.trim() is a and a.capacity_bytes == a.used_bytes == a.payload.numel()
    assert a.payload.untyped_storage().nbytes() == a.used_bytes and torch.equal(a.frames(idx, par, exp), want)


def test_store_reproduces_the_reference_fixture(dev):
    golden = load_golden('gen4_store')
    recordings = gen4_store_ref.fixture_recordings(golden)
    tab = gen4_store_ref.tables(recordings, 3, 2, (12, 16))
    store = data.Gen4PackedStore(recordings, 3, dev, sensor_hw=(12, 16), chunk=2)
    sums = np.concatenate([gen4_store_ref.bin_sums(r[1]) for r in recordings])
    assert np.array_equal(store.unpacked(0, 12).cpu().numpy(), sums)
    table, payload = ref.encode(sums)
    assert np.array_equal(store.rows.cpu().numpy(), table) and np.array_equal(store.payload.cpu().numpy(), payload)
    for k in ('rep_offsets', 'group_first', 'group_lo', 'boxes', 'group_start'):
        assert np.array_equal(getattr(store, k).cpu().numpy(), tab[k]), k
    exp = types.SimpleNamespace(Tm=3, Tl=1, input_size=(32, 48), test_size=(32, 48), num_classes=3)
    idx = torch.arange(7, device=dev)
    for params in (None, data.unscaled_params(7, (12, 16), dev), [(16, 12, 0, 0, 0)] * 7):
        got = store.frames(idx, params, exp).cpu().numpy()
        assert got.shape == (7, 1, 3, 2, 32, 48)
        assert np.array_equal(got[..., :12, :16].astype(np.float64), golden['slices'][:, 0][:, None])
        assert got.sum(dtype=np.float64) == golden['slices'].sum()                # zero padded to the canvas
    assert np.array_equal(store.frames(idx, None, exp, canvas_hw=(12, 16)).cpu().numpy().astype(np.float64), golden['slices'][:, 0][:, None])
    rs = np.random.RandomState(5)
    ids = np.array([1, 0, 5, 3, 2, 6, 4, 1], dtype=np.int64)
    par = np.array([data.jitter_params(12, 16, 32, 48, jitter=.3, rng=rs) for _ in ids], dtype=np.int32)
    got = store.frames(torch.from_numpy(ids).to(dev), par, exp).cpu().numpy()
    assert np.array_equal(got, gen4_store_ref.frames(recordings, tab, ids, 3, 32, 48, params=par)) and got.any()
    t = store.targets(torch.from_numpy(ids).to(dev), par, None, (32, 48))
    assert np.array_equal(t.cpu().numpy(), gen4_store_ref.targets(tab, ids, par, (12, 16), (32, 48))[0])


def test_build_stays_inside_its_bound(dev):
    """the device holds the arena, the table, one uploaded chunk and its u16 scratch (a fifth of the chunk at 10 bins): at most arena +
    table + 2 chunks of u8 + 1 MiB above what was allocated before.  80 representations of a 64 x 128 sensor: a build that also held the
    u16 form whole would lie above that bound"""
    H, W, R, per_chunk = 64, 128, 80, 4
    recs = data.synth_gen4_recordings(2, R // 2, (H, W), 10, 3, seed=4)
    chunk, table, u16 = per_chunk * 20 * H * W, R * 2 * H * 3 * 8, R * 2 * H * W * 2
    capacity = u16 * 5 // 8
    bound = capacity + table + 2 * chunk + (1 << 20)
    assert u16 + capacity + table + chunk > bound
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    store = data.Gen4PackedStore(recs, 3, dev, sensor_hw=(H, W), chunk=per_chunk, capacity_bytes=capacity)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    print(f'peak {peak} bytes above the baseline; arena {capacity}, table {table}, u8 chunk {chunk}, u16 store {u16}, used {store.used_bytes}')
    assert store.rows.numel() * 8 == table and store.used_bytes <= capacity == store.capacity_bytes and store.nbytes < u16
    assert peak <= bound


# ------------------------------------------------------------------------------------------------ loaders, trainer, capture
def test_loaders_with_packed_sums_yield_what_u16_yields(dev):
    a, p = small_exp(store_recordings=(2, 12)), small_exp(store_recordings=(2, 12), store_sums='packed')
    la, lp = data.Gen4StoreLoader(a, 4, seed=2), data.Gen4StoreLoader(p, 4, seed=2)
    assert type(la.store) is data.Gen4Store and type(lp.store) is data.Gen4PackedStore and len(la) == len(lp) == 3
    assert data.hist_store_for(p) is lp.store and data.hist_store_for(p, 'test') is not lp.store
    n = 0
    for (fa, ta), (fp, tp) in zip(la, lp):
        assert torch.equal(fa, fp) and torch.equal(ta, tp) and fa.any().item() and fa.shape == (4, 1, 3, 2, 32, 64)
        n += 1
    assert n == 3
    ids = [0, 5, 9, 2, 13, 7]
    ea, ep = (data.Gen4StoreEvalLoader(e, 4, ids, data.hist_store_for(e, 'test')) for e in (a, p))
    assert type(ep.store) is data.Gen4PackedStore and type(ea.store) is data.Gen4Store
    for (fa, la_, (ha, wa), ia), (fp, lp_, (hp, wp), ip) in zip(ea, ep):
        assert torch.equal(fa, fp) and fa.any().item() and torch.equal(ia, ip) and torch.equal(ha, hp) and torch.equal(wa, wp)
        assert all(torch.equal(x, y) for x, y in zip(la_, lp_)) and len(la_) == len(lp_)


def test_trainer_losses_equal_the_u16_stores(dev, tmp_path, monkeypatch):
    """two iterations of ``yolox.core.Trainer.train()`` at a 64 x 64 canvas, batch 2, fed by ``train_input = 'hist_store'`` with
    ``store_sums`` 'u16' and 'packed': the same frames, so the same losses bit for bit"""
    from yolox.exp import get_exp
    monkeypatch.setattr(ops, 'VERIFY_SMALL_INT', False)      # the suite's tag check reads the device: not inside a capture
    losses = {}
    for kind in ('u16', 'packed'):
        exp = get_exp(None, 'e-yolox-s')
        exp.merge(BASE_OPTS + ['input_size', '(64, 64)', 'test_size', '(64, 64)', 'data_name', 'gen4'])
        exp.max_epoch, exp.print_interval, exp.output_dir = 1, 1, str(tmp_path / kind)
        exp.train_input, exp.store_recordings, exp.store_sums = 'hist_store', (1, 8), kind
        torch.manual_seed(5)
        tr = exp.get_trainer(types.SimpleNamespace(batch_size=2, fp16=False, experiment_name='packed_store', ckpt=None, resume=False))
        tr.train()
        torch.cuda.set_stream(torch.cuda.default_stream())
        store = tr.train_loader.store
        assert type(store) is (data.Gen4PackedStore if kind == 'packed' else data.Gen4Store) and store.sensor_hw == (64, 64)
        assert len(tr.train_loader) == 2 and len(tr.log) == 2 and all(np.isfinite(r['loss']) for r in tr.log)
        losses[kind] = [r['loss'] for r in tr.log]
    print('losses', losses)
    assert losses['packed'] == losses['u16']


def test_frames_replay_from_a_captured_graph(dev):
    golden = load_golden('gen4_store')
    recordings = gen4_store_ref.fixture_recordings(golden)
    tab = gen4_store_ref.tables(recordings, 3, 2, (12, 16))
    store = data.Gen4PackedStore(recordings, 3, dev, sensor_hw=(12, 16), chunk=2).trim()
    exp = types.SimpleNamespace(Tm=3, Tl=1, input_size=(32, 48), test_size=(32, 48), num_classes=3)
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
