"""CPU-only tests of ``aggregation timesurface`` on the device front ends: the two latest-surface entry points are declared, exported and
bound and refuse bad arguments without a GPU, the checker (tests/agg_ts_ref.py) reproduces tests/golden/ncaltech_agg_timesurface.npz --
recorded from the reference's own read_ATIS / generate_slices / agrregate(aggregation='timesurface') -- exactly, and every chain function
and loader of ``eas_snn_amd.data`` refuses an aggregation whose frames the sampler cannot take, while 'micro_sum' stays what it was."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

import agg_ts_ref as ref
import eas_snn_amd
from eas_snn_amd import data, ops

NEW_ABI = ['eas_event_latest_surface_atis', 'eas_event_latest_surface_dat_ranges']
INVALID_ARG, UNSUPPORTED = -1, -2
P = 0x1000                                                           # a 16-byte aligned address nobody dereferences


@pytest.fixture(scope='module')
def cases():
    return ref.load_cases()


def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    eas_snn_amd._lib._bind_host_hip_runtime()
    handle = ctypes.CDLL(eas_snn_amd._lib.LIB_PATH)
    for n in NEW_ABI:
        assert n in declared, f'{n} is not declared in include/eas_hip.h'
        assert hasattr(handle, n), f'{n} is not exported by libeas_hip.so'
        assert n in eas_snn_amd._lib.PROTOTYPES, f'{n} is not in _lib.PROTOTYPES'
    lib = eas_snn_amd.hip_library()
    assert lib.eas_abi_version() == eas_snn_amd._lib.ABI_VERSION == 9                     # purely additive
    for n in ('event_latest_surface_atis', 'event_latest_surface_dat_ranges'):
        assert hasattr(ops, n)
    assert data.FRAME_AGGREGATIONS == ('micro_sum', 'timesurface') and data.ATIS_MEASURES == ('count', 'timesurface')


def test_bad_arguments_are_refused_before_any_launch():
    """no GPU here: a call that got as far as a launch could not answer EAS_ERR_INVALID_ARG"""
    lib = eas_snn_amd.hip_library()

    def atis(rec=P, off=P, out=P, ws=P, tau=10e3, nrec=10, B=1, Tl=1, Tm=4, H=36, W=48):
        return lib.eas_event_latest_surface_atis(rec, nrec, off, B, 0, 0, Tl, Tm, H, W, tau, out, None, None, ws, None)

    def dat(rec=P, ranges=P, out=P, tau=50e3, B=1, ns=4, H=24, W=32):
        return lib.eas_event_latest_surface_dat_ranges(rec, ranges, B, ns, H, W, tau, out, None, None)

    for call in (atis, dat):
        for tau in (0.0, -1.0, float('nan')):
            assert call(tau=tau) == INVALID_ARG, (call.__name__, tau)
        for dim in ('B', 'H', 'W'):
            for v in (0, -3):
                assert call(**{dim: v}) == INVALID_ARG, (call.__name__, dim, v)
        assert call(out=None) == INVALID_ARG and call(rec=None) == INVALID_ARG
    for dim in ('Tl', 'Tm'):
        for v in (0, -3):
            assert atis(**{dim: v}) == INVALID_ARG, (dim, v)
    assert dat(ns=0) == INVALID_ARG and dat(ns=-1) == INVALID_ARG and dat(ranges=None) == INVALID_ARG and dat(rec=P + 4) == INVALID_ARG
    assert atis(off=None) == INVALID_ARG and atis(ws=None) == INVALID_ARG and atis(ws=P + 8) == INVALID_ARG and atis(nrec=-1) == INVALID_ARG


def test_both_dat_range_entries_share_one_argument_rule():
    """The count entry and the latest-surface entry of .dat record ranges refuse the same arguments the same way, without a GPU: the sample
    is a block's y index in both, so a batch above 65535 is EAS_ERR_UNSUPPORTED.  That assertion on eas_event_histogram_dat_ranges is new
    with the shared host template: before it the entry went on to a launch that failed (here, without a GPU, with another error code)."""
    lib = eas_snn_amd.hip_library()

    def count(rec=P, ranges=P, out=P, B=1, ns=4, H=24, W=32):
        return lib.eas_event_histogram_dat_ranges(rec, ranges, B, ns, H, W, out, None, None)

    def latest(rec=P, ranges=P, out=P, B=1, ns=4, H=24, W=32):
        return lib.eas_event_latest_surface_dat_ranges(rec, ranges, B, ns, H, W, 50e3, out, None, None)

    for call in (count, latest):
        assert call(B=65536) == UNSUPPORTED, call.__name__
        for dim in ('B', 'ns', 'H', 'W'):
            for v in (0, -3):
                assert call(**{dim: v}) == INVALID_ARG, (call.__name__, dim, v)
        for bad in (dict(out=None), dict(rec=None), dict(ranges=None), dict(rec=P + 4)):
            assert call(**bad) == INVALID_ARG, (call.__name__, bad)
        assert call(B=65536, H=0) == INVALID_ARG, call.__name__            # a bad argument is reported before an unsupported size


@pytest.mark.parametrize('name', ref.CASES)
def test_checker_reproduces_the_reference_exactly(cases, name):
    """the same int64 subtraction, the same division and the same libm exp on both sides: equal bit for bit.  The checker reports a micro
    window of 0 exactly where the reference raised."""
    c = cases[name]
    assert c['frames'].dtype == np.float64 and c['frames'].shape == (len(c['bufs']), c['Tl'], c['Tm'], 2, c['H'], c['W'])
    for b, buf in enumerate(c['bufs']):
        got, oob, flags = ref.atis_latest_surface(buf, c['window'], c['Tl'], c['Tm'], c['H'], c['W'])
        assert oob == 0 and flags & ~ref.WINDOW0 == 0
        assert bool(flags & ref.WINDOW0) == bool(c['raises'][b]), f'{name}[{b}]'
        assert np.array_equal(got, c['frames'][b]), f'{name}[{b}]: {int((got != c["frames"][b]).sum())} elements differ'
        if c['raises'][b]:
            assert not got.any()
        else:
            assert (got > 0).all() and (got < 1).all() and (np.log(got) >= -100).all()


def test_fixture_holds_the_cases_it_is_meant_to(cases):
    assert [f'{n}[{b}]' for n in ref.CASES for b in np.flatnonzero(cases[n]['raises'])] == ['short_span_w0[0]']
    assert sum(len(c['bufs']) for c in cases.values()) == 23
    hot = cases[ref.HOT]
    raw = hot['bufs'][0].reshape(-1, 5)
    assert (raw[:, 1] == 240).sum() >= 3 and raw[0, 1] == 240 and hot['Tm'] == 4
    # the hot pixel is hit anew in every micro slice: it decays by less than the micro window from frame to frame, which a pixel nothing
    # touches (the least value of a frame: latest = 0) decays by
    ticks = ref.exponent_ticks(hot['frames'][0, 0])
    w = -np.diff(ticks.reshape(4, -1).min(axis=1))
    p, y, x = ref.HOT_PIXEL
    assert (w == w[0]).all() and w[0] > 0 and (np.diff(ticks[:, p, y, x]) > -w).all()
    # count frames, or the time-surface measure's, cannot pass for these: no element is zero
    assert all((c['frames'][c['raises'] == 0] > 0).all() for c in cases.values())
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'ncaltech_agg_timesurface.npz')) < 512 * 1024


def small_exp(**fields):
    return types.SimpleNamespace(Tl=1, Tm=4, img_size=(36, 48), input_size=(64, 64), test_size=(64, 64), window=None, num_classes=2, **fields)


@pytest.mark.parametrize('aggregation', ['voxel_grid', 'voxel_cube'])
def test_every_chain_and_loader_refuses_frames_the_sampler_cannot_take(aggregation):
    """before any device work: the arguments that would hold tensors are None"""
    dims, match = (1, 4, (36, 48), (64, 64)), "'micro_sum' and 'timesurface'.*two channels per micro slice"
    exp = small_exp(aggregation=aggregation)
    calls = [lambda: data.atis_to_frames(None, None, dims, None, aggregation=aggregation),
             lambda: data.atis_to_frames(None, None, exp, None),
             lambda: data.atis_to_frames(None, None, exp, None, measure='timesurface'),
             lambda: data.events_to_frames(None, 4, (24, 32), (32, 32), aggregation=aggregation),
             lambda: data.events_to_frames_augmented(None, 4, (24, 32), (32, 32), None, aggregation=aggregation),
             lambda: data.dat_ranges_to_frames(None, None, 4, (24, 32), (32, 32), None, aggregation=aggregation),
             lambda: data.SyntheticEventLoader(exp, 2),
             lambda: data.SyntheticEvalLoader(exp, 2, range(4))]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match=match) as err:
            call()
        assert repr(aggregation) in str(err.value), i
    with pytest.raises(ValueError, match="'micro_sum' and 'timesurface'"):
        data.check_aggregation('event_sum')


def test_micro_sum_and_a_missing_field_behave_as_before():
    """an experiment without ``aggregation`` is 'micro_sum': the measure check and its messages are the ones test_cpu_ncaltech_ts.py pins"""
    exp = small_exp(measure='voxel')
    assert not hasattr(exp, 'aggregation')
    with pytest.raises(ValueError, match="measure 'voxel'.*'count' and 'timesurface'"):
        data.atis_to_frames(None, None, exp, None)
    with pytest.raises(ValueError, match="measure 'voxel'"):
        data.atis_to_frames(None, None, small_exp(measure='voxel', aggregation='micro_sum'), None)
    with pytest.raises(ValueError, match="measure 'voxel'"):
        data.atis_to_frames(None, None, (1, 4, (36, 48), (64, 64)), None, measure='voxel', aggregation='micro_sum')
    assert data.exp_aggregation(exp) == 'micro_sum' and data.exp_aggregation(small_exp(aggregation='timesurface')) == 'timesurface'
    from yolox.exp import get_exp
    assert data.exp_aggregation(get_exp(None, 'e-yolox-s')) == 'micro_sum'


def test_timesurface_does_not_consult_the_measure():
    """as in the reference, which computes its measure function for this aggregation and does not use it: the call gets past the measure
    check and stops at the operator, which has no CPU path"""
    rec, off = torch.zeros(50, dtype=torch.uint8), torch.tensor([0, 10])
    for exp in (small_exp(measure='voxel', aggregation='timesurface'), small_exp(aggregation='timesurface')):
        with pytest.raises(eas_snn_amd._lib.EasHipError, match='GPU only'):
            data.atis_to_frames(rec, off, exp, None)
    with pytest.raises(eas_snn_amd._lib.EasHipError, match='GPU only'):
        data.atis_to_frames(rec, off, (1, 4, (36, 48), (64, 64)), None, measure='voxel', aggregation='timesurface')
