"""CPU-only tests of the 1 Mpx front end's host side: ``eas_stacked_hist_frames`` is declared, exported and bound and refuses bad arguments
before any launch; ``data.gen4_rescale_labels`` / ``gen4_raw_boxes`` equal tests/golden/gen4_front.npz -- recorded from the reference's own
``RVTGEN4Dataset.extract_labels`` and ``__getitem__`` (scripts/gen_golden_gen4.py) -- exactly; ``data.rvt_first_index`` and the checker
(tests/gen4_ref.py) reproduce every case of tests/golden/stacked_hist.npz (the reference's generate_slices) bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

import gen4_ref
import eas_snn_amd
from eas_snn_amd import data, ops

INVALID, UNSUPPORTED = -1, -2


def stacked_hist_cases():
    """(key, store u8 [R, 2*nbins, H, W], time, num_slice, expected float64 [1, num_slice, 2, H, W]) of tests/golden/stacked_hist.npz"""
    g = load_golden('stacked_hist')
    for key in [str(k) for k in g['cases']]:
        name, spec = key.split('/')
        time, num_slice = int(spec[1:spec.index('_')]), int(spec[spec.index('_n') + 2:])
        yield key, g[f'{name}/data'], time, num_slice, g[key]


@pytest.fixture(scope='module')
def front():
    return load_golden('gen4_front')


def test_entry_point_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    eas_snn_amd._lib._bind_host_hip_runtime()
    handle = ctypes.CDLL(eas_snn_amd._lib.LIB_PATH)
    n = 'eas_stacked_hist_frames'
    assert n in declared, f'{n} is not declared in include/eas_hip.h'
    assert hasattr(handle, n), f'{n} is not exported by libeas_hip.so'
    assert n in eas_snn_amd._lib.PROTOTYPES, f'{n} is not in _lib.PROTOTYPES'
    assert eas_snn_amd._lib.ABI_VERSION == 9 and eas_snn_amd.hip_library().eas_abi_version() == 9          # purely additive
    assert hasattr(ops, 'stacked_hist_frames') and hasattr(ops, 'stacked_hist_event_sum')
    for name in ('rvt_to_frames', 'rvt_first_index', 'gen4_rescale_labels', 'gen4_raw_boxes', 'SyntheticStackedHistLoader'):
        assert hasattr(data, name)


def test_bad_arguments_are_refused_before_any_launch():
    """every call below returns from the argument checks: no device is touched (the pointers are made-up addresses)"""
    fn = eas_snn_amd.hip_library().eas_stacked_hist_frames
    good = dict(store=0x10000, R=7, first=0x20000, lo=0x30000, params=0x40000, B=2, Tm=3, nbins=10, H=18, W=32, Hc=32, Wc=48, out=0x50000,
                flags=0x60000)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a['store'], a['R'], a['first'], a['lo'], a['params'], a['B'], a['Tm'], a['nbins'], a['H'], a['W'], a['Hc'], a['Wc'], a['out'],
                  a['flags'], None)
    for kw in (dict(store=None), dict(first=None), dict(out=None),                                         # the three that must exist
               dict(store=0x10001), dict(out=0x50004), dict(first=0x20004), dict(lo=0x30004), dict(params=0x40002), dict(flags=0x60001),
               dict(R=0), dict(R=-1), dict(B=0), dict(B=-3), dict(Tm=0), dict(nbins=0), dict(H=0), dict(W=-1), dict(Hc=0), dict(Wc=0)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(Wc=40), dict(Wc=8), dict(nbins=256), dict(W=1 << 17)):
        assert call(**kw) == UNSUPPORTED, kw
    assert call(store=None, Wc=40) == INVALID                                                              # bad arguments first


def test_event_sum_refuses_bad_arguments_before_any_launch():
    """every call below returns from the argument checks of ``eas_stacked_hist_event_sum``: no device is touched (the pointers are made-up
    addresses)"""
    fn = eas_snn_amd.hip_library().eas_stacked_hist_event_sum
    good = dict(hist=0x10000, n_valid=0x20000, B=2, Tm=3, nbins=10, H=18, W=32, Hc=32, Wc=48, out=0x50000)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a['hist'], a['n_valid'], a['B'], a['Tm'], a['nbins'], a['H'], a['W'], a['Hc'], a['Wc'], a['out'], None)
    for kw in (dict(hist=None), dict(out=None), dict(hist=0x10001), dict(out=0x50004), dict(n_valid=0x20002),
               dict(Hc=17), dict(Wc=16), dict(W=40, Wc=32), dict(B=-1), dict(Tm=0), dict(nbins=0), dict(H=0), dict(W=0)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(Wc=40), dict(nbins=256)):
        assert call(**kw) == UNSUPPORTED, kw
        assert call(B=0, **kw) == UNSUPPORTED, kw                                                          # limits before the empty batch
    assert call(hist=None, Wc=40) == INVALID                                                               # bad arguments first
    assert call(B=0) == 0 and call(B=0, n_valid=None) == 0                                                  # an empty batch is no work


def test_cpu_tensors_raise():
    import torch
    with pytest.raises(eas_snn_amd._lib.EasHipError):
        ops.stacked_hist_frames(torch.zeros(3, 20, 4, 16, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), 2, 32, 32)


def test_rescale_and_raw_boxes_equal_the_reference(front):
    labels, first, img_size = front['labels'], front['objframe_idx_2_label_idx'], tuple(int(v) for v in front['img_size'])
    assert labels.dtype == np.float32 and img_size == (360, 640)
    ends = list(first[1:]) + [len(labels)]                                   # the last object frame is open-ended (rvt_gen4.py:400-401)
    for factor in (1, 2):
        rows, off, boxes = front[f'dsf{factor}/rows'], front[f'dsf{factor}/offsets'], front[f'dsf{factor}/raw_boxes']
        assert len(off) == len(first) + 1
        for k, (a, b) in enumerate(zip(first, ends)):
            before = labels[a:b].copy()
            got = data.gen4_rescale_labels(labels[a:b], factor, img_size)
            want = rows[off[k]:off[k + 1]]
            assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), (factor, k)
            assert np.array_equal(labels[a:b], before)                       # the input is left alone
            box = data.gen4_raw_boxes(got)
            assert box.dtype == np.float32 and np.array_equal(box, boxes[off[k]:off[k + 1]]), (factor, k)
    # the fixture holds the cases it is meant to: boxes across the border (clipped at factor 2, untouched at factor 1), boxes dropped,
    # an empty frame, rows in the open-ended last frame
    n1, n2 = np.diff(front['dsf1/offsets']), np.diff(front['dsf2/offsets'])
    assert list(n1) == [5, 4, 0, 2] and list(n2) == [5, 1, 0, 2]
    b1, b2 = front['dsf1/raw_boxes'], front['dsf2/raw_boxes']
    assert b1[:, 2].max() > 1280 and b1[:, 0].min() < 0 and b2[:, 2].max() == 639 and b2[:, 3].max() == 359 and b2[:, :2].min() == 0
    assert (b2[:, :4] % 1 == 0.5).any()                                      # halves survive: float32 rows, no rounding
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'gen4_front.npz')) < 200 * 1024
    assert data.gen4_rescale_labels(np.zeros((0, 7)), 2, img_size).shape == (0, 7)


def test_first_index_reproduces_the_fixture_starts():
    seen = {}
    for key, store, time, num_slice, want in stacked_hist_cases():
        obj2repr = np.arange(len(store), dtype=np.int64)                     # the fixture's objframe_idx_2_repr_idx is the identity
        first = data.rvt_first_index(obj2repr, time, num_slice)
        assert first == time + 1 - num_slice
        seen[(time, num_slice)] = int(first)
    assert seen[(0, 3)] == -2 and seen[(1, 4)] == -2 and seen[(3, 1)] == 3 and seen[(2, 3)] == 0
    # arrays of labels, a recording that does not start the store, a representation index that is not the label index
    obj2repr = np.array([2, 2, 5, 9], dtype=np.int64)
    assert list(data.rvt_first_index(obj2repr, np.array([0, 3, 2]), 4, offset=100)) == [99, 106, 102]
    import torch
    got = data.rvt_first_index(torch.from_numpy(obj2repr), torch.tensor([0, 3, 2]), 4, offset=100)
    assert got.dtype == torch.int64 and got.tolist() == [99, 106, 102]


def test_checker_reproduces_generate_slices_bit_for_bit():
    n = 0
    for key, store, time, num_slice, want in stacked_hist_cases():
        H, W = store.shape[-2:]
        first = [data.rvt_first_index(np.arange(len(store)), time, num_slice)]
        got, flags = gen4_ref.frames(store, first, num_slice, H, W, nbins=store.shape[1] // 2)
        assert got.dtype == np.float32 and got.shape == (1,) + want.shape and flags[0] == 0, key
        assert np.array_equal(got[0].astype(np.float64), want), key
        # on a larger canvas: zero padding bottom / right
        Hc, Wc = H + 3, (W + 31) // 32 * 32
        pad, _ = gen4_ref.frames(store, first, num_slice, Hc, Wc, nbins=store.shape[1] // 2)
        assert np.array_equal(pad[0, ..., :H, :W].astype(np.float64), want) and pad.sum(dtype=np.float64) == want.sum(), key
        n += 1
    assert n == 20


def test_checker_rules_for_lo_end_of_store_and_clipping():
    rng = np.random.default_rng(5)
    store = rng.integers(0, 256, (5, 6, 4, 16), dtype=np.uint8)
    sums = store.reshape(5, 2, 3, 4, 16).sum(2).astype(np.float32)
    got, flags = gen4_ref.frames(store, [-1, 2, 3, 4, 9], 3, 4, 16, nbins=3, lo=[0, 3, 0, 0, 0])
    assert list(flags) == [0, 0, 1, 1, 1]
    assert not got[0, 0, 0].any() and np.array_equal(got[0, 0, 1:], sums[0:2])
    assert not got[1, 0, 0].any() and np.array_equal(got[1, 0, 1:], sums[3:5])            # index 2 < lo = 3: the neighbour stays out
    assert np.array_equal(got[2, 0, :2], sums[3:5]) and not got[2, 0, 2].any()            # index 5 >= R
    assert np.array_equal(got[3, 0, 0], sums[4]) and not got[3, 0, 1:].any() and not got[4].any()
    # identity size, pasted so that it sticks out at the bottom right / top left: the visible part, then the flip
    out, _ = gen4_ref.frames(store, [0], 1, 4, 16, nbins=3, params=[(16, 4, 10, 2, 0)])
    assert np.array_equal(out[0, 0, 0, :, 2:, 10:], sums[0][:, :2, :6]) and out.sum(dtype=np.float64) == sums[0][:, :2, :6].sum(dtype=np.float64)
    neg, _ = gen4_ref.frames(store, [0], 1, 4, 16, nbins=3, params=[(16, 4, -3, -1, 1)])
    assert np.array_equal(neg[0, 0, 0, :, :3, ::-1][..., :13], sums[0][:, 1:, 3:])
    assert not gen4_ref.frames(store, [0], 1, 4, 16, nbins=3, params=[(0, 4, 0, 0, 0)])[0].any()
    assert not gen4_ref.frames(store, [0], 1, 4, 16, nbins=3, params=[(16, -2, 0, 0, 0)])[0].any()
