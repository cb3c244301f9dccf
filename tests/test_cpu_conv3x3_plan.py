"""The 3x3 convolution planners, asked without a GPU (eas_conv_fwd_plan, eas_conv_dgrad_s2_plan, eas_conv_fwd_group_tile_plan: the launch's own
decision, handed back from the planners' common exit): every row of tests/conv3x3_cases.py lands on exactly the instance and run-time form it
promises, and a walk over the search box stated there finds no instance, run-time form or edge that has no row -- the only exemptions are
the LEFT_OUT tables, whose every entry carries its reason and is asserted never to be reached.  tests/test_gpu_conv3x3_instances.py launches
the same rows: one table checked from both sides."""
import collections

import pytest

import eas_snn_amd
import conv3x3_cases as K

EAS_ERR_UNSUPPORTED = -2


@pytest.fixture(scope='module')
def lib():
    return eas_snn_amd.hip_library()


def test_every_forward_row_lands_on_its_instance_and_form(lib):
    for key, shape in K.CASES:
        s, terms = key[0], key[1]
        for xt in ((3,) if terms == 3 else (1, 2)):          # one term: fp32 small integers and spike planes plan alike
            rc, p = K.fwd_plan(lib, shape, s, xt)
            assert rc == 0, (key, shape, xt)
            assert K.fwd_key(shape, s, terms, p) == key, (shape, xt, K.fwd_key(shape, s, terms, p), key)
            wvm, wvn, wn = K.TILES[p.cand]
            assert (p.wvm, p.wvn, p.wn, p.threads) == (wvm, wvn, wn, 64 * wvm * wvn), (key, shape)
            Ho, Wo = K.out_size(shape[3], shape[4], s)
            assert p.grid_z == p.parts and p.grid_y == -(-((shape[2] + 31) // 32) // wvm) and p.grid_x == -(-shape[0] * Ho // p.RT), (key, shape)
            assert 0 < p.lds_bytes <= 160 * 1024 and p.RT * (Wo // p.parts) <= 32 * wn * wvn and p.bpi == 0, (key, shape)
            # the queries that existed before answer by the same plan
            assert lib.eas_conv_fwd_supported(*shape, 3, s, xt) == 1
            assert lib.eas_conv_fwd_stats_blocks(*shape, 3, s, xt) == p.grid_x * p.parts
    assert len({k for k, _ in K.CASES}) >= 140


def test_forward_walk_finds_nothing_without_a_row(lib):
    """every (instance, run-time form) the planner chooses anywhere in the box has a row; every edge a tile meets anywhere in the box it
    meets in a row; nothing in LEFT_OUT is ever chosen; LEFT_OUT and the rows together are the 168 compiled LM = 0 instances"""
    rows = {k for k, _ in K.CASES}
    met = collections.defaultdict(set)
    for key, shape in K.CASES:
        _, p = K.fwd_plan(lib, shape, key[0], key[1])
        met[(key[0], key[3])] |= K.fwd_edges(shape, key[0], p)
    nq, seen, reach = 0, set(), collections.defaultdict(set)
    for shape, s in K.fwd_box():
        plans = {}
        for xt in (3, 1, 2):
            rc, p = K.fwd_plan(lib, shape, s, xt)
            nq += 1
            assert rc == 0, ('the box has a refused geometry', shape, s, xt)
            terms = 3 if xt == 3 else 1
            key = plans[xt] = K.fwd_key(shape, s, terms, p) + (p.RT, p.grid_x)
            seen.add(key[:8])
            reach[(s, p.cand)] |= K.fwd_edges(shape, s, p)
        assert plans[1] == plans[2], ('planes and fp32 one-term inputs plan differently', shape, s)
    assert nq > 30000
    assert seen <= rows, sorted(seen - rows)
    assert rows <= seen, sorted(rows - seen)          # (the rows are box shapes)
    reached = {k[:4] for k in seen}
    assert not reached & set(K.LEFT_OUT), sorted(reached & set(K.LEFT_OUT))
    every = {(s, t, v, c) for s in (1, 2) for t in (3, 1) for v in (4, 2) for c in range(14)}
    assert reached | set(K.LEFT_OUT) == every
    assert all(len(reason) > 20 and ratio >= 1.0 for reason, ratio in K.LEFT_OUT.values())          # every entry carries its reason
    n = lambda keys: sum(2 if k[1] == 1 else 1 for k in keys)          # a one-term key is two compiled instances
    assert n(every) == 168 and n(reached) == 71 and n(K.LEFT_OUT) == 97
    for sc in reach:
        assert reach[sc] <= met[sc], (sc, sorted(reach[sc] - met[sc]))
    assert not any('parts8' in e for e in reach.values())          # eight column parts: not in this box


def test_every_stride2_input_gradient_row_lands_on_its_instance(lib):
    for key, shape in K.S2D_CASES:
        rc, p = K.s2d_plan(lib, shape)
        assert rc == 0 and K.s2d_key(shape, p) == key, (shape, K.s2d_key(shape, p), key)
        wvm, wvn, wn = K.S2D_TILES[p.cand]
        assert (p.wvm, p.wvn, p.wn, p.threads) == (wvm, wvn, wn, 64 * wvm * wvn) and p.parts == 1 and p.single == 0
        assert p.grid_y == -(-((shape[1] + 31) // 32) // wvm) and p.grid_z == 1
        assert lib.eas_conv_dgrad_s2_supported(*shape) == 1


def test_stride2_input_gradient_walk_finds_nothing_without_a_row(lib):
    rows = {k for k, _ in K.S2D_CASES}
    met = collections.defaultdict(set)
    for key, shape in K.S2D_CASES:
        met[key[0]] |= K.s2d_edges(shape, K.s2d_plan(lib, shape)[1])
    seen, reach, nq = set(), collections.defaultdict(set), 0
    for shape in K.s2d_box():
        rc, p = K.s2d_plan(lib, shape)
        nq += 1
        assert (rc == 0) == bool(lib.eas_conv_dgrad_s2_supported(*shape)), shape
        if rc:
            assert rc == EAS_ERR_UNSUPPORTED, shape
            continue
        seen.add(K.s2d_key(shape, p))
        reach[p.cand] |= K.s2d_edges(shape, p)
    assert nq > 8000 and seen == rows, (sorted(seen - rows), sorted(rows - seen))
    reached = {k[:2] for k in seen}
    assert not reached & set(K.S2D_LEFT_OUT)
    assert reached | set(K.S2D_LEFT_OUT) == {(c, v) for c in range(7) for v in (4, 2, 1)} and len(reached) == 6
    assert all(len(r) > 20 for r in K.S2D_LEFT_OUT.values())
    for c in reach:
        assert reach[c] <= met[c], (c, sorted(reach[c] - met[c]))


def test_every_group_lands_on_its_tile(lib):
    assert sorted(c for c, _, _ in K.GROUP_CASES.values()) == [0, 1, 2, 3]
    for name, (cand, probs, vecs) in K.GROUP_CASES.items():
        rc, plans = K.group_plan(lib, probs)
        assert rc == 0, name
        first = 0
        for p, q, vec in zip(plans, probs, vecs):
            assert (p.cand, p.vec, (p.wvm, p.wvn, p.wn)) == (cand, vec, K.GROUP_TILES[cand]), (name, q)
            assert p.grid_x == -(-q[0] * q[3] // p.RT) and p.parts == 1 and p.single == 0, (name, q)
            first += p.grid_x
        assert all(p.grid_z == first for p in plans), name
        assert len({q[1] for q in probs}) == 3 and len({q[3:] for q in probs}) == 3
    assert any(len(set(v)) > 1 for _, _, v in K.GROUP_CASES.values())          # a group mixes VEC 2 and VEC 4


def test_refused_geometries_and_the_1x1_family(lib):
    from eas_snn_amd import _lib
    out = _lib.EasConvPlan()
    for NI, Cin, Cout, H, W, s in K.REFUSED:
        for xt in (3, 1, 2):
            assert K.fwd_plan(lib, (NI, Cin, Cout, H, W), s, xt)[0] == EAS_ERR_UNSUPPORTED, (NI, Cin, Cout, H, W, s, xt)
            assert lib.eas_conv_fwd_supported(NI, Cin, Cout, H, W, 3, s, xt) == 0
    import ctypes
    assert lib.eas_conv_fwd_plan(2, 16, 24, 8, 8, 1, 1, 3, ctypes.byref(out)) == EAS_ERR_UNSUPPORTED          # 1x1: a family of its own
    assert lib.eas_conv_fwd_supported(2, 16, 24, 8, 8, 1, 1, 3) == 1
    assert lib.eas_conv_fwd_plan(2, 16, 24, 8, 8, 3, 1, 3, None) == -1 and lib.eas_conv_dgrad_s2_plan(2, 16, 24, 8, 8, None) == -1
    assert lib.eas_conv_dgrad_s2_plan(1, 8, 8, 4, 10, ctypes.byref(out)) == EAS_ERR_UNSUPPORTED          # odd Wo
    assert K.group_plan(lib, [(1, 12, 16, 8, 12)] * 2)[0] == EAS_ERR_UNSUPPORTED
