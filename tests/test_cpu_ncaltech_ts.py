"""CPU-only tests of the N-Caltech101 front end's measure 'timesurface': the new entry points are declared, exported and bound and refuse bad
arguments without a GPU, the checker (tests/ncaltech_ts_ref.py) reproduces tests/golden/ncaltech_timesurface.npz -- recorded from the
reference's own read_ATIS / generate_slices / agrregate with measure='timesurface' --, the fixture holds what it is meant to, the kernel's
2^-48 quantisation stays inside the end-to-end bounds of tests/test_gpu_ncaltech_ts.py, and ``data.atis_to_frames`` refuses a measure it does
not have."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT

import ncaltech_ref
import ncaltech_ts_ref as ts_ref
import eas_snn_amd
from eas_snn_amd import data, ops

TS_ABI = ['eas_event_timesurface_atis_workspace_bytes', 'eas_event_timesurface_atis_capacity', 'eas_event_timesurface_atis',
          'eas_frames_letterbox_f64']
INVALID_ARG = -1


@pytest.fixture(scope='module')
def cases():
    return ts_ref.load_cases()


@pytest.fixture(scope='module')
def restated(cases):
    """per case: (frames, quantised frames, counts) of the checker, every recording stacked -- computed once"""
    out = {}
    for name, c in cases.items():
        runs = [[ts_ref.atis_timesurface_frames(buf, c['window'], c['Tl'], c['Tm'], c['H'], c['W'], quantised=q) for buf in c['bufs']]
                for q in (False, True)]
        for r in runs[0] + runs[1]:
            assert r[2] == 0 and r[3] == 0          # no out-of-sensor event, no flag: the reference raises on anything else
        out[name] = (np.stack([r[0] for r in runs[0]]), np.stack([r[0] for r in runs[1]]), np.stack([r[1] for r in runs[0]]))
    return out


def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    eas_snn_amd._lib._bind_host_hip_runtime()
    handle = ctypes.CDLL(eas_snn_amd._lib.LIB_PATH)
    for n in TS_ABI:
        assert n in declared, f'{n} is not declared in include/eas_hip.h'
        assert hasattr(handle, n), f'{n} is not exported by libeas_hip.so'
        assert n in eas_snn_amd._lib.PROTOTYPES, f'{n} is not in _lib.PROTOTYPES'
    lib = eas_snn_amd.hip_library()
    assert lib.eas_abi_version() == eas_snn_amd._lib.ABI_VERSION == 9                     # purely additive
    for n in ('event_timesurface_atis', 'frames_letterbox'):
        assert hasattr(ops, n)
    assert data.ATIS_MEASURES == ('count', 'timesurface')


def test_workspace_query_and_capacity_answer_on_the_host():
    lib = eas_snn_amd.hip_library()
    q, qc = lib.eas_event_timesurface_atis_workspace_bytes, lib.eas_event_histogram_atis_workspace_bytes
    for nrec, B, Tl in ((0, 1, 1), (1, 1, 1), (257, 3, 2), (150_000, 64, 1), (1 << 31, 64, 8)):
        extra = q(nrec, B, Tl) - qc(nrec, B, Tl)
        assert 4 * B * Tl <= extra < 4 * B * Tl + 16 and q(nrec, B, Tl) % 16 == 0          # the t_target rows, behind the count entry's part
    assert q(-1, 1, 1) == 0 and q(10, 0, 1) == 0 and q(10, 1, 0) == 0
    # a weight of 1 is 2^48 in an unsigned 64-bit bin
    assert lib.eas_event_timesurface_atis_capacity() == ts_ref.CAPACITY == 65535


def test_bad_arguments_are_refused_before_any_launch():
    """no GPU here: a call that got as far as a launch could not answer EAS_ERR_INVALID_ARG"""
    lib = eas_snn_amd.hip_library()
    P = 0x1000                                                       # a 16-byte aligned address nobody dereferences

    def call(rec=P, off=P, out=P, ws=P, tau=500e3, nrec=10):
        return lib.eas_event_timesurface_atis(rec, nrec, off, 1, 0, 0, 1, 4, 36, 48, tau, out, None, None, ws, None)

    for tau in (0.0, -1.0, float('nan')):
        assert call(tau=tau) == INVALID_ARG, tau
    assert call(rec=None) == INVALID_ARG and call(off=None) == INVALID_ARG and call(out=None) == INVALID_ARG and call(ws=None) == INVALID_ARG
    assert call(ws=P + 8) == INVALID_ARG and call(nrec=-1) == INVALID_ARG
    f = lib.eas_frames_letterbox_f64
    assert f(None, P, 1, 1, 1, 36, 48, 64, 64, P, None) == INVALID_ARG and f(P, None, 1, 1, 1, 36, 48, 64, 64, P, None) == INVALID_ARG
    assert f(P, P, 1, 1, 1, 36, 48, 64, 64, None, None) == INVALID_ARG and f(P, P, 2, 1, 1, 36, 48, 64, 64, P, None) == INVALID_ARG
    assert f(P, P, 0, 0, 1, 36, 48, 64, 64, P, None) == INVALID_ARG


@pytest.mark.parametrize('name', ts_ref.CASES)
def test_checker_reproduces_the_reference(cases, restated, name):
    """the same libm tanh on both sides and the same order of adds in a bin: 1e-13 relative"""
    want = cases[name]['frames']
    got, _, counts = restated[name]
    assert want.dtype == np.float64 and want.shape == got.shape
    assert np.array_equal(want == 0, counts == 0) and np.array_equal(got == 0, counts == 0)
    assert (np.abs(got - want) <= 1e-13 * np.abs(want)).all(), float(np.abs(got - want).max())


def test_fixture_holds_the_cases_it_is_meant_to(cases, restated):
    for name in ts_ref.CASES:
        c = cases[name]
        counts = restated[name][2]
        assert c['H'] == 36 and c['W'] == 48 and len(c['bufs']) <= 3
        hit = counts > 0
        mean_weight = c['frames'][hit] / counts[hit]
        assert (mean_weight > 0.85).all() and (mean_weight <= 1).all()
        # count frames cannot pass for these: every occupied bin misses its count by more than 1e-6 per event
        assert ((counts[hit] - c['frames'][hit]) >= 1e-6 * counts[hit]).all(), name
    hot = cases[ts_ref.HOT]
    assert np.array_equal(hot['counts'], restated[ts_ref.HOT][2][0][None])
    raw = hot['bufs'][0].reshape(-1, 5)
    t, x, y, p = ncaltech_ref.decode_atis(hot['bufs'][0])
    assert len(hot['bufs']) == 1 and len(t) >= 900 and len(raw) > 4 * 256
    at = np.unravel_index(int(hot['counts'].argmax()), hot['counts'].shape)          # (b, k, q, p, y, x)
    assert hot['counts'][at] >= 600
    on_pixel = np.flatnonzero((x == at[5]) & (y == at[4]) & (p == at[3]))
    rec_index = np.flatnonzero(raw[:, 1] != 240)[on_pixel]                          # record indices of the events on the hot pixel
    overflow = np.flatnonzero(raw[:, 1] == 240)
    assert ((overflow > rec_index[0]) & (overflow < rec_index[-1])).sum() >= 3       # overflow records between them
    assert len(set((rec_index // 256).tolist())) >= 4                                # spread over at least four chunks of 256 records
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'ncaltech_timesurface.npz')) < 256 * 1024


@pytest.mark.parametrize('interp', ['cubic', 'linear'])
def test_quantised_weights_stay_inside_the_end_to_end_bounds(cases, restated, interp):
    """What tests/test_gpu_ncaltech_ts.py asserts of ``data.atis_to_frames(measure='timesurface')``, confirmed here for the kernel's
    arithmetic restated (weights rounded to 2^-48, integer bin sums): every bin within count * 2^-47 of the fixture, every letterboxed
    fp32 element within one fp32 ulp of the letterboxed fixture, at least 99 % of them equal."""
    tiny = float(np.finfo(np.float32).tiny)
    for name in ts_ref.CASES:
        want, (_, quant, counts) = cases[name]['frames'], restated[name]
        assert (np.abs(quant - want) <= counts * 2.0 ** -47).all() and not quant[counts == 0].any()
        par = ts_ref.case_params(len(want))
        a = ts_ref.letterbox(want, par, *ts_ref.CANVAS, interp).astype(np.float32).astype(np.float64)
        b = ts_ref.letterbox(quant, par, *ts_ref.CANVAS, interp).astype(np.float32).astype(np.float64)
        assert (np.abs(b - a) <= 2.0 ** -23 * np.maximum(np.abs(a), tiny)).all(), (name, float(np.abs(b - a).max()))
        assert (a == b).mean() >= 0.99, (name, float((a == b).mean()))


def test_linear_restatement_has_the_properties_of_inter_linear():
    for n_src, n_dst in ((48, 64), (36, 48), (48, 40), (36, 30), (5, 17)):
        idx, c = ts_ref.linear_taps(n_src, n_dst)
        assert c.dtype == np.float32 and idx.min() >= 0 and idx.max() <= n_src - 1 and (c >= 0).all()
        assert np.abs(c.astype(np.float64).sum(1) - 1).max() <= 2.0 ** -25          # 1 - f rounds once, to a value below 1
    const = np.full((2, 36, 48), 3.25)
    assert np.array_equal(ts_ref.resize_linear(const, 64, 48), np.full((2, 48, 64), 3.25))
    img = np.random.default_rng(0).random((3, 36, 48))
    assert np.array_equal(ts_ref.resize_linear(img, 48, 36), img)
    box = ts_ref.letterbox(img[:, None], [(48, 36, 5, 3, 0)] * 3, 64, 64, 'linear')
    assert np.array_equal(box[:, 0, 3:39, 5:53], img) and np.array_equal(ts_ref.letterbox(img[:, None], [(48, 36, 5, 3, 1)] * 3, 64, 64, 'linear'),
                                                                          box[..., ::-1])


def test_atis_to_frames_refuses_a_measure_it_does_not_have():
    dims = (1, 4, (36, 48), (64, 64))
    with pytest.raises(ValueError, match="'count' and 'timesurface'"):
        data.atis_to_frames(None, None, dims, None, measure='voxel')
    exp = types.SimpleNamespace(Tl=1, Tm=4, img_size=(36, 48), input_size=(64, 64), window=None, measure='voxel')
    with pytest.raises(ValueError, match='voxel'):
        data.atis_to_frames(None, None, exp, None)
