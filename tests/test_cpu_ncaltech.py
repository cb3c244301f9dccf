"""CPU-only tests of the N-Caltech101 front end's host side: the three entry points are declared, exported and bound, the workspace query
answers without a GPU, the checker (tests/ncaltech_ref.py) reproduces every case of tests/golden/ncaltech_atis.npz -- recorded from the
reference's own read_ATIS / generate_slices / agrregate -- exactly, the ATIS encoder round-trips, and the cubic resize has the properties
of OpenCV's INTER_CUBIC (parity against cv2 unpinned: no cv2 here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden, split_cases

import ncaltech_ref
import eas_snn_amd
from eas_snn_amd import data, ops

ATIS_ABI = ['eas_event_histogram_atis_workspace_bytes', 'eas_event_histogram_atis', 'eas_counts_letterbox_ex']
CASES = ['plain_1x4', 'window0_2x3', 'negwin_1x8', 'negwin_hi_2x3', 'overflow_1x4', 'overflow_negwin_2x3', 'overflow_1x8', 'short_span_w0',
         'polarity_1x4', 'polarity_2x3']


def case_window(case):
    return tuple(int(v) for v in case['window']) if int(case['has_window']) else None


def case_recordings(case):
    off = case['offsets']
    return [case['bytes'][5 * off[b]:5 * off[b + 1]] for b in range(len(off) - 1)]


@pytest.fixture(scope='module')
def golden():
    cases = split_cases(load_golden('ncaltech_atis'))
    assert sorted(cases) == sorted(CASES)
    return cases


def test_atis_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    eas_snn_amd._lib._bind_host_hip_runtime()
    handle = ctypes.CDLL(eas_snn_amd._lib.LIB_PATH)
    for n in ATIS_ABI:
        assert n in declared, f'{n} is not declared in include/eas_hip.h'
        assert hasattr(handle, n), f'{n} is not exported by libeas_hip.so'
        assert n in eas_snn_amd._lib.PROTOTYPES, f'{n} is not in _lib.PROTOTYPES'
    assert eas_snn_amd._lib.ABI_VERSION == 9                      # purely additive
    for n in ('event_histogram_atis', 'counts_letterbox'):
        assert hasattr(ops, n)
    for n in ('encode_atis', 'synth_atis_batch', 'atis_to_frames'):
        assert hasattr(data, n)


def test_workspace_query_answers_on_the_host_and_is_monotone():
    q = eas_snn_amd.hip_library().eas_event_histogram_atis_workspace_bytes
    assert q(0, 1, 1) > 0
    sizes = [0, 1, 255, 256, 257, 4096, 150_000, 64 * 150_000, 1 << 31]
    for B, Tl in ((1, 1), (64, 1), (64, 2)):
        got = [q(n, B, Tl) for n in sizes]
        assert all(g > 0 for g in got) and got == sorted(got) and got[-1] > got[0]
    assert q(1000, 1, 1) < q(1000, 2, 1) < q(1000, 64, 1) and q(1000, 64, 1) < q(1000, 64, 2) < q(1000, 64, 8)
    assert q(-1, 1, 1) == 0 and q(10, 0, 1) == 0 and q(10, 1, 0) == 0


@pytest.mark.parametrize('name', CASES)
def test_checker_reproduces_the_reference_exactly(golden, name):
    case = golden[name]
    Tl, Tm, H, W = (int(case[k]) for k in ('Tl', 'Tm', 'H', 'W'))
    assert case['bytes'].dtype == np.uint8 and case['frames'].dtype == np.int32
    recs = case_recordings(case)
    assert case['frames'].shape == (len(recs), Tl, Tm, 2, H, W)
    for b, buf in enumerate(recs):
        counts, oob, flags = ncaltech_ref.atis_frames(buf, case_window(case), Tl, Tm, H, W)
        assert np.array_equal(counts, case['frames'][b]), (name, b)
        assert oob == 0 and flags == 0          # the reference raises on anything else


def test_fixture_holds_the_cases_it_is_meant_to(golden):
    """the places where a kernel can go wrong are really in the file"""
    assert {case_window(golden[n]) is None for n in CASES} == {True, False}
    assert any(case_window(golden[n]) == (0, 0) for n in CASES) and any((case_window(golden[n]) or (0,))[0] < 0 for n in CASES)
    assert {(int(golden[n]['Tl']), int(golden[n]['Tm'])) for n in CASES} >= {(1, 4), (2, 3), (1, 8)}
    t = ncaltech_ref.decode_atis(case_recordings(golden['plain_1x4'])[0])[0]
    assert (t == t[-1]).sum() >= 3                                                         # several events on the last timestamp
    y = [r.reshape(-1, 5)[:, 1] for r in case_recordings(golden['overflow_1x4'])]
    assert y[0][0] == 240 and y[0][-1] == 240 and (y[0][1:-1] == 240).any()               # overflow first, last and in the middle
    assert (y[1][:2] == 240).all() and (y[2][-2:] == 240).all()                            # runs of them
    assert not golden['short_span_w0']['frames'][0].any() and golden['short_span_w0']['frames'][1].any()      # w == 0
    f = golden['polarity_1x4']['frames']
    assert f[0, :, :, 1].sum() > 5 * f[0, :, :, 0].sum() and f[1, :, :, 0].sum() > 5 * f[1, :, :, 1].sum()
    for n in CASES:
        assert int(golden[n]['H']) <= 36 and int(golden[n]['W']) <= 48
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'ncaltech_atis.npz')) < 256 * 1024


def test_encode_decode_round_trip():
    rng = np.random.default_rng(3)
    n = 500
    t = np.sort(rng.integers(8192 * 6, 400_000, n))
    x, p = rng.integers(0, 256, n), rng.integers(0, 2, n)
    y = rng.integers(0, 255, n)
    y[y >= 240] += 1                                               # every y but 240
    for ov in ((), (0,), (n,), (0, 0, 17, 250, 250, n, n)):
        buf = data.encode_atis(t, x, y, p, overflow_before=ov)
        assert buf.dtype == np.uint8 and buf.shape == (5 * (n + len(ov)),)
        assert (buf.reshape(-1, 5)[:, 1] == 240).sum() == len(ov)
        td, xd, yd, pd = ncaltech_ref.decode_atis(buf)
        assert np.array_equal(td, t) and np.array_equal(xd, x) and np.array_equal(yd, y) and np.array_equal(pd, p)
    with pytest.raises(AssertionError):
        data.encode_atis([5], [0], [0], [0], overflow_before=(0,))       # the raw time would be negative
    buf, off = data.synth_atis_batch(3, 2000, 36, 48, seed=1)
    assert buf.dtype == np.uint8 and off.dtype == np.int64 and off[0] == 0 and 5 * off[-1] == len(buf) and len(off) == 4
    for b in range(3):
        rec = buf[5 * off[b]:5 * off[b + 1]]
        td, xd, yd, _ = ncaltech_ref.decode_atis(rec)
        assert len(td) == 2000 and (np.diff(td) >= 0).all() and td[-1] < 300_000 and xd.max() < 48 and yd.max() < 36
        assert (rec.reshape(-1, 5)[:, 1] == 240).sum() == 4              # 300 ms: the marks at 65536 * (1..4)


def test_cubic_weights_and_resize_properties():
    for n_src, n_dst in ((24, 32), (18, 24), (24, 13), (18, 9), (180, 192), (240, 256), (5, 17)):
        idx, c = ncaltech_ref.cubic_taps(n_src, n_dst)
        assert c.dtype == np.float32 and idx.min() >= 0 and idx.max() <= n_src - 1
        # c3 = 1 - c0 - c1 - c2 is three float32 subtractions of results below 1.25: each rounds by at most 2^-24 * 1.25
        assert np.abs(c.astype(np.float64).sum(1) - 1).max() <= 3 * 1.25 * 2.0 ** -24
    # Where the scale is a dyadic fraction (3/4, 3/2, 2, 1/2 below) every fraction f is a multiple of 1/8, the cubic polynomials are exact
    # in float32 and the weights sum to exactly 1: a constant image comes back constant.  (At other scales the sum is 1 only to float32
    # rounding, as asserted above, and so is a constant image.)
    const = np.full((2, 18, 24), 7.0)
    for nw, nh in ((32, 24), (16, 12), (12, 9), (48, 36), (32, 9)):
        got = ncaltech_ref.resize_cubic(const, nw, nh)
        assert got.shape == (2, nh, nw) and np.abs(got - 7.0).max() <= 1e-12
    rng = np.random.default_rng(0)
    img = rng.integers(0, 9, (3, 18, 24))
    same = ncaltech_ref.resize_cubic(img, 24, 18)
    assert same.dtype == np.float64 and np.array_equal(same, img)
    box = ncaltech_ref.letterbox_cubic(img[:, None], [(24, 18, 5, 3, 0)] * 3, 24, 32)       # identity size, integer shift: a copy
    assert np.array_equal(box[:, 0, 3:21, 5:29], img) and box.sum() == img.sum()
    flipped = ncaltech_ref.letterbox_cubic(img[:, None], [(24, 18, 5, 3, 1)] * 3, 24, 32)
    assert np.array_equal(flipped, box[..., ::-1])
    assert data.letterbox_params(180, 240, 192, 256) == (256, 192, 0, 0, 0)
