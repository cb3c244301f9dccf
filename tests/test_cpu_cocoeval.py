"""CPU-only tests of the device COCO evaluation's host side: the eas_cocoeval_* entry points are declared and bound, the checker
(tests/cocoeval_ref.py) reproduces every case of tests/golden/cocoeval.npz -- recorded from the reference's own native module -- bit for bit,
``ops.coco_summarize`` forms the statistics and the text of ``COCOeval.summarize``, the switch is a context field, CPU tensors raise, and the
evaluator on a CPU model takes the route it took before."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, split_cases

import cocoeval_ref
import eas_snn_amd
from eas_snn_amd import ops

COCOEVAL_ABI = ['eas_cocoeval_supported', 'eas_cocoeval_workspace_bytes', 'eas_cocoeval_keys', 'eas_cocoeval_match', 'eas_cocoeval_accumulate']
CASES = ['empties', 'maxdets', 'ties', 'areas', 'thresholds', 'large']
INPUTS = ('det_img', 'det_cls', 'det_box', 'det_score', 'gt_img', 'gt_cls', 'gt_box')

LARGE_LINES = '''\
 Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.513
 Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.712
 Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=100 ] = 0.561
 Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = 0.245
 Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = 0.532
 Average Precision  (AP) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 0.366
 Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.461
 Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets= 10 ] = 0.738
 Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.882
 Average Recall     (AR) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = 0.973
 Average Recall     (AR) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = 0.883
 Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 1.000'''


@pytest.fixture(scope='module')
def golden():
    cases = split_cases(load_golden('cocoeval'))
    assert sorted(cases) == sorted(CASES)
    return cases


def test_cocoeval_entry_points_are_declared_and_bound():
    src = open(os.path.join(ROOT, 'include', 'eas_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(eas_[a-z0-9_]+)\s*\(', src))
    for n in COCOEVAL_ABI:
        assert n in declared, f'{n} is not declared in include/eas_hip.h'
        assert n in eas_snn_amd._lib.PROTOTYPES, f'{n} is not in _lib.PROTOTYPES'
    assert eas_snn_amd._lib.ABI_VERSION == 9                      # purely additive


def test_limits_are_answered_on_the_host():
    assert ops.coco_eval_supported(6_000_000, 250_000, 60_000, 2, max_gt=64)          # a Gen1 test split
    assert not ops.coco_eval_supported(10, 10, 4, 2, max_gt=65)                        # ground truths per (image, category)
    assert not ops.coco_eval_supported(10, 10, 4, 2, T=17) and not ops.coco_eval_supported(10, 10, 4, 2, T=16, A=5)
    assert not ops.coco_eval_supported(10, 10, 4, 2, R=129) and not ops.coco_eval_supported(10, 10, 4, 2, M=9)
    assert not ops.coco_eval_supported(10, 10, (1 << 24) + 1, 1) and not ops.coco_eval_supported(1 << 31, 10, 4, 2)
    assert ops.coco_eval_supported(0, 0, 0, 1)


@pytest.mark.parametrize('name', CASES)
def test_checker_reproduces_the_reference_binary_bit_for_bit(golden, name):
    case = golden[name]
    for k in ('det_box', 'det_score', 'gt_box'):
        assert case[k].dtype == np.float32
    got = cocoeval_ref.evaluate(*[case[k] for k in INPUTS], case['num_images'], case['num_classes'])
    assert got['precision'].shape == case['precision'].shape == (10, 101, int(case['num_classes']), 4, 3)
    assert np.array_equal(got['precision'], case['precision']) and np.array_equal(got['recall'], case['recall'])


def test_fixture_holds_the_cases_it_is_meant_to(golden):
    """the places where a kernel can go wrong are really in the file"""
    c = golden['maxdets']
    assert np.bincount(c['det_img'])[0] > 100                                          # (b) the cut at 100
    c = golden['ties']
    assert len(np.unique(c['det_score'])) <= 3 < len(c['det_score'])                   # (c)
    c = golden['areas']
    areas = (c['gt_box'][:, 2].astype(np.float64) * c['gt_box'][:, 3]).tolist()
    assert areas.count(32.0 ** 2) >= 2 and areas.count(96.0 ** 2) >= 2                 # (d) inclusive bounds
    c = golden['thresholds']
    ious = [cocoeval_ref.bb_iou([float(v) for v in d], [float(v) for v in g]) for d in c['det_box'] for g in c['gt_box']]
    assert 0.5 in ious and 0.75 in ious                                                # (e) exactly at a threshold
    with_ids_from_one = cocoeval_ref.evaluate(*[c[k] for k in INPUTS], c['num_images'], c['num_classes'], gt_id=np.arange(1, len(c['gt_box']) + 1))
    assert not np.array_equal(with_ids_from_one['recall'], c['recall'])                # (i) the annotation with id 0 is matched
    c = golden['empties']
    assert (c['precision'][:, :, 2] == -1).all() and (c['precision'][:, :, 1, 0] == 0).all()      # (h)
    c = golden['large']
    assert (c['det_cls'] == 0).sum() > 2500 and int(c['num_images']) == 40             # (j) several chunks of the accumulate walk


@pytest.mark.parametrize('name', CASES)
def test_summarize_gives_the_means_numpy_gives(golden, name):
    case = golden[name]
    stats, lines = ops.coco_summarize(dict(precision=case['precision'], recall=case['recall']))
    want = cocoeval_ref.summarize(case['precision'], case['recall'])
    assert stats.dtype == np.float64 and stats.tolist() == want.tolist() and len(lines) == 12
    p = case['precision'][:, :, :, 0, 2]
    assert stats[0] == np.mean(p[p > -1])
    p = case['precision'][5, :, :, 0, 2]
    assert stats[2] == np.mean(p[p > -1])
    r = case['recall'][:, :, 0, 0]
    assert stats[6] == np.mean(r[r > -1])
    r = case['recall'][:, :, 3, 2]
    assert stats[11] == (np.mean(r[r > -1]) if (r > -1).any() else -1)
    # torch tensors are accepted as well (what ops.coco_eval returns)
    stats_t, _ = ops.coco_summarize(dict(precision=torch.from_numpy(case['precision']), recall=torch.from_numpy(case['recall'])))
    assert stats_t.tolist() == stats.tolist()


def test_the_twelve_lines(golden):
    case = golden['large']
    _, lines = ops.coco_summarize(dict(precision=case['precision'], recall=case['recall']))
    assert '\n'.join(lines) == LARGE_LINES


def test_default_tables_are_pycocotools():
    d = ops.coco_default_params()
    assert len(d['iou_thr']) == 10 and len(d['rec_thr']) == 101 and tuple(d['max_dets']) == (1, 10, 100)
    assert d['iou_thr'].tolist() == np.linspace(.5, .95, 10).tolist() and d['rec_thr'].tolist() == np.linspace(0, 1, 101).tolist()
    assert d['area_rng'].tolist() == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]


def test_switch_is_a_context_field_and_defaults_on():
    assert 'EAS_DEVICE_AP' not in os.environ or os.environ['EAS_DEVICE_AP'] in ('0', '1')
    assert ops.ctx.device_ap is (os.environ.get('EAS_DEVICE_AP', '1') == '1')


def test_cpu_tensors_raise(golden):
    case = golden['areas']
    with pytest.raises(eas_snn_amd._lib.EasHipError, match='GPU only'):
        ops.coco_eval(*[torch.from_numpy(np.ascontiguousarray(case[k])) for k in INPUTS], int(case['num_images']), int(case['num_classes']))


class _ToyModel(torch.nn.Module):
    """a fixed decoded head output; a CPU model, so the evaluator's device route is not taken"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))

    def forward(self, x):
        B = x.shape[0]
        out = torch.zeros(B, 6, 7)
        for a in range(6):
            out[:, a, 0], out[:, a, 1] = 40. + 30 * a, 50. + 10 * a
            out[:, a, 2:4] = 30.
            out[:, a, 4] = 0.9 * self.w
            out[:, a, 5 + a % 2] = 0.8
        return out


class _ToyLoader:
    batch_size = 2
    dataset = type('D', (), {'map_val': True, 'random_aug': False, 'class_names': ['a', 'b']})()

    def __len__(self):
        return 2

    def __iter__(self):
        for ids in ([0, 1], [2]):
            yield (torch.zeros(len(ids), 1, 4, 2, 8, 10), [torch.tensor([[25., 35., 30., 30., 0.]]) for _ in ids],
                   (torch.full((len(ids),), 240), torch.full((len(ids),), 304)), torch.tensor(ids))


def test_evaluator_on_a_cpu_model_behaves_as_before(monkeypatch):
    import yolox.evaluators.event_evaluator as EV
    from oracle import postprocess_ref

    def cpu_postprocess(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, class_agnostic=False):
        out = postprocess_ref.postprocess(prediction.cpu().numpy(), num_classes, conf_thre, nms_thre, class_agnostic)
        return [None if o is None else torch.from_numpy(o) for o in out]

    def must_not_run(*a, **k):
        raise AssertionError('the device AP route was taken for a CPU model')
    monkeypatch.setattr(EV, 'postprocess', cpu_postprocess)
    monkeypatch.setattr(ops, 'coco_eval', must_not_run)
    ev = EV.EventEvaluator(_ToyLoader(), (256, 320), 0.3, 0.5, 2)
    (ap50_95, ap50, summary), outputs = ev.evaluate(_ToyModel(), return_outputs=True)
    assert sorted(outputs) == [0, 1, 2] and len(outputs[0]['scores']) == 6 and summary.startswith('Average forward time:')
    try:
        import pycocotools  # noqa: F401
        assert ap50_95 >= 0 and ' Average Precision  (AP)' in summary
    except ImportError:
        assert ap50_95 is None and ap50 is None
        assert summary.endswith('18 detections on 3 images; pycocotools is not installed: AP not computed\n')
        assert 'declined' not in summary


def test_evaluator_names_the_reason_when_the_kernels_decline():
    """65 ground truths in one (image, category): the limits are asked on the host before anything touches a device, the summary says why, and
    the earlier route answers"""
    import yolox.evaluators.event_evaluator as EV
    ev = EV.EventEvaluator(_ToyLoader(), (256, 320), 0.3, 0.5, 2)
    gt_dict = {0: {'bboxes': [[0., 0., 10., 10.]] * 65, 'category_ids': [0] * 65, 'width': 304, 'height': 240}}
    data = [{'image_id': 0, 'category_id': 0, 'bbox': [0., 0., 10., 10.], 'score': 0.5, 'segmentation': []}]
    a, b, summary = ev.evaluate_prediction(data, gt_dict, torch.tensor([1.0, 1.0, 1.0]), device=torch.device('cuda:0'))
    assert ev.last_coco is None
    assert 'AP on the device declined: 1 detections, 65 ground truths (65 in one image and class)' in summary
    try:
        import pycocotools  # noqa: F401
        assert a >= 0 and ' Average Precision  (AP)' in summary
    except ImportError:
        assert a is None and b is None
        assert summary.endswith('1 detections on 1 images; pycocotools is not installed: AP not computed\n')
