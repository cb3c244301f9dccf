"""CPU-only tests of the Prophesee-protocol evaluation's host side: tests/golden/psee.npz -- recorded from the reference's own filter, time
matching and native COCO evaluation -- holds the cases it is meant to; the numpy route of yolox/utils/psee_loader reproduces every case's flat
rows exactly and the checker (tests/cocoeval_ref.py) the recorded precision / recall / statistics from them; the eas_psee_* entry points are
declared and bound; ``get_evaluator`` hands out PSEEEvaluator exactly when the sample names carry label times; the buffer of
PropheseeEvaluator."""
import os
import re
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, split_cases

import cocoeval_ref
import eas_snn_amd
from eas_snn_amd import ops

PSEE_ABI = ['eas_psee_mark', 'eas_psee_windows', 'eas_psee_expand']
CASES = ['filters_gen1', 'filters_gen4', 'filters_gen4_half', 'rounding', 'windows', 'large', 'samples']
ROWS = ('det_img', 'det_cls', 'det_box', 'det_score', 'gt_img', 'gt_cls', 'gt_box', 'gt_id', 'image_file', 'image_t')
COCO_IN = ('det_img', 'det_cls', 'det_box', 'det_score', 'gt_img', 'gt_cls', 'gt_box')


@pytest.fixture(scope='module')
def golden():
    cases = split_cases(load_golden('psee'))
    assert sorted(cases) == sorted(CASES)
    return cases


def box_lists(case):
    """the case's two box sets as lists of structured arrays, one per file"""
    from yolox.utils.psee_loader.records import BBOX_DTYPE
    out = []
    for side in ('gt', 'dt'):
        n = len(case[side + '_t'])
        a = np.zeros(n, BBOX_DTYPE)
        a['t'], a['class_id'] = case[side + '_t'], case[side + '_cls']
        for j, k in enumerate('xywh'):
            a[k] = case[side + '_box'][:, j]
        a['class_confidence'] = case['dt_score'] if side == 'dt' else 1.0
        off = case[side + '_offsets']
        out.append([a[off[f]:off[f + 1]] for f in range(len(off) - 1)])
    return out


def host_rows(case):
    from yolox.utils.psee_loader.evaluation import SKIP_TS, thresholds
    from yolox.utils.psee_loader.io.box_filtering import filter_boxes
    from yolox.utils.psee_loader.metrics.coco_eval import match_rows
    diag, side = thresholds(str(case['camera']), bool(case['downsampled_by_2']))
    gts, dts = box_lists(case)
    gts, dts = [filter_boxes(g, SKIP_TS, diag, side) for g in gts], [filter_boxes(d, SKIP_TS, diag, side) for d in dts]
    return match_rows(gts, dts, int(case['time_tol'])), (sum(len(g) for g in gts), sum(len(d) for d in dts))


def test_psee_entry_points_are_declared_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    for n in PSEE_ABI:
        assert n in declared, f'{n} is not declared in include/eas_hip.h'
        assert n in eas_snn_amd._lib.PROTOTYPES, f'{n} is not in _lib.PROTOTYPES'
    assert eas_snn_amd._lib.ABI_VERSION == 9                      # purely additive
    for n in ('psee_match', 'psee_eval', 'psee_thresholds'):
        assert hasattr(ops, n)
    assert ops.psee_thresholds('gen1') == (30, 10) and ops.psee_thresholds('gen4') == (60, 20) and ops.psee_thresholds('gen4', True) == (30, 10)
    assert ops.psee_thresholds('gen1', True) == (15, 5)
    with pytest.raises(ValueError):
        ops.psee_thresholds('gen3')


def test_cpu_tensors_raise(golden):
    case = golden['samples']
    gt = tuple(torch.from_numpy(case[k]) for k in ('gt_t', 'gt_box', 'gt_cls', 'gt_offsets'))
    dt = tuple(torch.from_numpy(case[k]) for k in ('dt_t', 'dt_box', 'dt_cls', 'dt_score', 'dt_offsets'))
    with pytest.raises(eas_snn_amd._lib.EasHipError, match='GPU only'):
        ops.psee_match(gt, dt)


def _decisions(w, h, diag):
    """per row: the float32 decision with separately rounded products and sum, the decision in real numbers, the two fma forms"""
    w, h = np.asarray(w, np.float32), np.asarray(h, np.float32)
    thr = np.float32(diag * diag)
    f32 = (w * w + h * h) >= thr
    real = np.array([Fraction(float(a)) ** 2 + Fraction(float(b)) ** 2 >= diag * diag for a, b in zip(w, h)])
    w64, h64 = w.astype(np.float64), h.astype(np.float64)               # a product of two float32 is exact in double, and so is its sum
    fma_a = (w64 * w64 + (h * h).astype(np.float64)).astype(np.float32) >= thr       # with a float32 of this size (checked below)
    fma_b = (h64 * h64 + (w * w).astype(np.float64)).astype(np.float32) >= thr
    for a, b, hh in zip(w64, h64, (h * h).astype(np.float64)):
        assert Fraction(a * a + hh) == Fraction(a) ** 2 + Fraction(hh)
    return f32, real, fma_a, fma_b


def test_fixture_holds_the_cases_it_is_meant_to(golden):
    for name, camera, half, K in (('filters_gen1', 'gen1', 0, 2), ('filters_gen4', 'gen4', 0, 3), ('filters_gen4_half', 'gen4', 1, 3)):
        c = golden[name]
        D, S = ops.psee_thresholds(camera, bool(half))
        assert str(c['camera']) == camera and int(c['downsampled_by_2']) == half and c['precision'].shape[2] == K
        for side in ('gt', 'dt'):
            t, w, h = c[side + '_t'], c[side + '_box'][:, 2], c[side + '_box'][:, 3]
            assert (t == 500000).any() and (t == 500001).any()
            assert ((w == 0.6 * D) & (h == 0.8 * D)).any() and (w == S).any() and (h == S).any()          # exactly on the thresholds
            assert (w == S - 0.25).any() and (h == S - 0.25).any()
        assert ((c['dt_box'] == 0).all(1) & (c['dt_score'] == 0)).any()                                    # the placeholder row
        assert 500001 in c['out_image_t'] and 500000 not in c['out_image_t']
        assert ((c['out_gt_box'][:, 2] == 0.6 * D) & (c['out_gt_box'][:, 3] == 0.8 * D)).any()
        assert (c['out_gt_box'][:, 2:] >= S).all() and (c['out_det_box'][:, 2:] >= S).all()
        assert sorted(np.unique(c['gt_cls']).tolist()) == list(range(K))
    c = golden['rounding']
    f32, real, fma_a, fma_b = _decisions(c['gt_box'][:, 2], c['gt_box'][:, 3], 30)
    assert (f32 != real).sum() >= 8 and ((f32 != fma_a) | (f32 != fma_b)).sum() >= 8
    assert f32.any() and not f32.all() and int(f32.sum()) == int(c['kept'][0])
    c = golden['windows']
    assert len(c['out_det_img']) > int(c['kept'][1])                                                       # duplicated detections
    assert len(np.unique(c['out_image_t'])) < len(c['out_image_t']) and c['out_image_t'].max() > 2 ** 32
    assert (c['gt_t'] == 1_500_000).any() and 1_500_000 not in c['out_image_t']                            # all ground truths filtered away
    F = len(c['gt_offsets']) - 1
    per_file = np.bincount(c['out_image_file'], minlength=F)
    gt_n, dt_n = np.diff(c['gt_offsets']), np.diff(c['dt_offsets'])
    assert ((gt_n > 0) & (dt_n == 0) & (per_file > 0)).any()                                               # ground truth, no detections
    assert ((gt_n > 0) & (dt_n > 0) & (per_file == 0)).any() and ((gt_n == 0) & (dt_n > 0)).any()          # detections, no image
    assert ((gt_n == 0) & (dt_n == 0)).any() and np.bincount(c['out_gt_img']).max() >= 3
    tol = int(c['time_tol'])
    first = int(c['out_image_t'][0])
    for edge in (first - tol - 1, first - tol, first + tol, first + tol + 1):
        assert (c['dt_t'] == edge).any()
    assert np.diff(c['out_image_t'])[0] == 60000
    c = golden['large']
    assert len(c['gt_offsets']) - 1 == 40 and len(c['dt_t']) >= 3000 and int(c['num_images']) > 700
    assert np.bincount(c['out_det_img']).max() > 256 and len(c['out_det_img']) > int(c['kept'][1])
    assert np.diff(c['dt_offsets']).max() > 1024
    assert np.bincount(c['out_gt_img'].astype(np.int64) * 3 + c['out_gt_cls']).max() <= 64
    c = golden['samples']
    assert len(c['gt_offsets']) - 1 == 64 and int(c['num_images']) == 58
    assert all(len(np.unique(c['gt_t'][a:b])) == 1 for a, b in zip(c['gt_offsets'][:-1], c['gt_offsets'][1:]))
    for name in CASES:
        if name != 'rounding':
            c = golden[name]
            for k in ('gt_box', 'dt_box'):
                assert c[k].dtype == np.float32 and (c[k] * 4 == np.round(c[k] * 4)).all() and (c[k] < 512).all() and (c[k] >= 0).all()
        assert (golden[name]['dt_score'] * 4096 == np.round(golden[name]['dt_score'] * 4096)).all()


@pytest.mark.parametrize('name', CASES)
def test_host_route_reproduces_the_reference_rows(golden, name):
    case = golden[name]
    rows, kept = host_rows(case)
    assert list(kept) == case['kept'].tolist() and rows['num_images'] == int(case['num_images'])
    for k in ROWS:
        assert rows[k].dtype == case['out_' + k].dtype and np.array_equal(rows[k], case['out_' + k]), k
    assert rows['gt_id'].tolist() == list(range(1, len(rows['gt_id']) + 1))


@pytest.fixture(scope='module')
def checked(golden):
    """the checker's arrays per case, computed once"""
    out = {}
    for name in CASES:
        c = golden[name]
        out[name] = cocoeval_ref.evaluate(*[c['out_' + k] for k in COCO_IN], int(c['num_images']), c['precision'].shape[2], gt_id=c['out_gt_id'])
    return out


@pytest.mark.parametrize('name', CASES)
def test_checker_reproduces_the_reference_binary_on_the_rows(golden, checked, name):
    case, got = golden[name], checked[name]
    assert np.array_equal(got['precision'], case['precision']) and np.array_equal(got['recall'], case['recall'])
    stats = cocoeval_ref.summarize(got['precision'], got['recall'])
    assert stats[:6].tolist() == case['stats'].tolist()
    s2, _ = ops.coco_summarize(dict(precision=case['precision'], recall=case['recall']))
    assert s2[:6].tolist() == case['stats'].tolist()
    assert (case['precision'] > -1).any()


def test_annotation_ids_from_one_matter(golden):
    """with ids 0.. the detection matched to the first annotation would not count: the rows carry 1..G"""
    c = golden['windows']
    zero_based = cocoeval_ref.evaluate(*[c['out_' + k] for k in COCO_IN], int(c['num_images']), 2)
    assert not np.array_equal(zero_based['recall'], c['recall'])


def test_filter_boxes_and_evaluate_list_on_the_host(golden, monkeypatch):
    from yolox.utils.psee_loader.evaluation import evaluate_list
    from yolox.utils.psee_loader.io.box_filtering import filter_boxes
    from yolox.utils.psee_loader.metrics import coco_eval as M
    case = golden['filters_gen1']
    gts, dts = box_lists(case)
    kept = filter_boxes(gts[0], int(5e5), 30, 10)
    assert kept.dtype == gts[0].dtype and len(kept) == int(case['kept'][0]) - 1 and (kept['t'] > 500000).all()
    monkeypatch.setattr(M, 'device_route', lambda: None)
    import yolox.utils.psee_loader.evaluation as E
    monkeypatch.setattr(E, 'device_route', lambda: None)
    seen = {}

    def fake_ap(rows, classes, height, width):
        seen.update(rows=rows, classes=classes)
        return None
    monkeypatch.setattr(M, 'host_ap', fake_ap)
    out = evaluate_list(dts, gts, 240, 304, camera='gen1')
    assert out == {k: None for k in ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L')} and seen['classes'] == ('car', 'pedestrian')
    for k in ROWS:
        assert np.array_equal(seen['rows'][k], case['out_' + k]), k
    evaluate_list(dts, gts, 240, 304, camera='gen1', apply_bbox_filters=False)
    assert len(seen['rows']['gt_img']) == len(case['gt_t'])


def test_prophesee_evaluator_buffer(golden, monkeypatch):
    import yolox.utils.psee_loader.evaluator as EV
    ev = EV.PropheseeEvaluator('gen1', False)
    assert not ev.has_data()
    with pytest.warns(UserWarning, match='empty'):
        assert ev.evaluate_buffer(240, 304) is None
    gts, dts = box_lists(golden['samples'])
    with pytest.raises(AssertionError):
        ev.add_labels(gts[0])                                      # a list of arrays, not an array
    ev.add_labels(gts[:10])
    ev.add_predictions(dts[:10])
    ev.add_labels(gts[10:])
    ev.add_predictions(dts[10:])
    assert ev.has_data() and len(ev._buffer[ev.LABELS]) == len(ev._buffer[ev.PREDICTIONS]) == 64
    got = {}
    monkeypatch.setattr(EV, 'evaluate_list', lambda **kw: got.update(kw) or {'AP': 0.5})
    assert ev.evaluate_buffer(240, 304) == {'AP': 0.5}
    assert got['camera'] == 'gen1' and got['downsampled_by_2'] is False and got['apply_bbox_filters'] is True and got['height'] == 240
    assert got['gt_boxes_list'] is ev._buffer[ev.LABELS] and got['result_boxes_list'] is ev._buffer[ev.PREDICTIONS]
    ev.reset_buffer()
    assert not ev.has_data() and ev._buffer == {ev.LABELS: [], ev.PREDICTIONS: []}
    with pytest.raises(AssertionError):
        EV.PropheseeEvaluator('gen3', False)


def _exp(*extra):
    from yolox.exp import get_exp
    exp = get_exp(None, 'e-yolox-s')
    exp.merge(['num_classes', '2', 'input_size', '(64,96)', 'test_size', '(64,96)'] + list(extra))
    exp.eval_samples = 8
    return exp


def test_get_evaluator_routing():
    from yolox.evaluators import EventEvaluator, PSEEEvaluator
    exp = _exp('data_name', 'gen1', 'eval_proph', 'True')
    with pytest.warns(RuntimeWarning, match='PSEEEvaluator.*no label time'):
        ev = exp.get_evaluator(2, False)
    assert type(ev) is EventEvaluator and ev.dataloader.dataset.sample_names[3] == 'synthetic_000003'
    exp = _exp('data_name', 'gen1', 'eval_proph', 'True')
    exp.eval_label_period_us = 200000
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ev = exp.get_evaluator(2, False)
    assert type(ev) is PSEEEvaluator and isinstance(ev, EventEvaluator)
    assert ev.evaluator.dataset == 'gen1' and ev.evaluator.downsample_by_2 is False and ev.snn_reset == exp.use_spike
    assert [ev.get_time_from_name(n) for n in ev.dataloader.dataset.sample_names] == [i * 200000 for i in range(8)]
    exp = _exp('data_name', 'gen4', 'eval_proph', 'True', 'num_classes', '3')
    exp.eval_label_period_us = 1000
    ev = exp.get_evaluator(2, False)
    assert type(ev) is PSEEEvaluator and ev.evaluator.dataset == 'gen4' and ev.evaluator.downsample_by_2 is True
    exp = _exp('data_name', 'ncaltech101', 'eval_proph', 'True')
    exp.eval_label_period_us = 200000
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert type(exp.get_evaluator(2, False)) is EventEvaluator
    exp = _exp('data_name', 'gen1')                                # eval_proph not set: label times in the names change nothing
    exp.eval_label_period_us = 200000
    assert type(exp.get_evaluator(2, False)) is EventEvaluator


def test_records_of_the_evaluator():
    """convert_to_gt_format / convert_to_prophesee_format: the 40-byte record, the all-zero row for an image without detections, xywh on
    the sensor and obj * cls as the score; the outputs are not modified"""
    from yolox.evaluators import PSEEEvaluator
    from yolox.utils import xyxy2xywh
    from yolox.utils.psee_loader.records import BBOX_DTYPE
    assert BBOX_DTYPE.itemsize == 40
    ev = PSEEEvaluator(None, (64, 96), 0.01, 0.5, 2, dataset='GEN1')
    out = torch.tensor([[8., 4., 40., 36., 0.5, 0.25, 1.], [1., 2., 31., 42., 0.75, 0.5, 0.]])
    keep = out.clone()
    rows = ev.convert_to_gt_format([out, None], (torch.tensor([60, 60]), torch.tensor([100, 100])))
    assert torch.equal(out, keep) and rows[1].tolist() == [[0.0] * 6]
    scale = min(64 / 60.0, 96 / 100.0)
    want = xyxy2xywh(keep[:, :4] / scale)
    assert torch.equal(rows[0][:, :4], want) and rows[0][:, 4].tolist() == [1.0, 0.0] and rows[0][:, 5].tolist() == [0.125, 0.375]
    recs = ev.convert_to_prophesee_format(rows, ['rec_a_a1500000', 'x_a700'])
    assert recs[0].dtype == BBOX_DTYPE and recs[0]['t'].tolist() == [1500000, 1500000] and recs[1]['t'].tolist() == [700]
    assert recs[0]['w'].tolist() == want[:, 2].tolist() and recs[0]['class_id'].tolist() == [1, 0]
    assert recs[0]['class_confidence'].tolist() == [0.125, 0.375] and recs[1]['w'].tolist() == [0.0]
