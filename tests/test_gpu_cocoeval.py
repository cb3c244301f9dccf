"""GPU tests of the device COCO evaluation (``ops.coco_eval``, the eas_cocoeval kernels): every case of tests/golden/cocoeval.npz -- recorded
from the reference's own native module -- bit for bit, empty inputs, determinism and graph replay, the limits, and the evaluator end to end."""
import numpy as np
import pytest
import torch

from conftest import load_golden, split_cases

import cocoeval_ref

pytestmark = pytest.mark.gpu

BASE_OPTS = ['T', '3', 'embedding', 'arsnn', 'num_classes', '2', 'spike_attach', 'True', 'thresh', '1', 'readout', 'sum',
             'embedding_depth', '2', 'embedding_ksize', '5', 'write_zero', 'True', 'spike_fn', 'atan']
CASES = ['empties', 'maxdets', 'ties', 'areas', 'thresholds', 'large']
INPUTS = ('det_img', 'det_cls', 'det_box', 'det_score', 'gt_img', 'gt_cls', 'gt_box')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    import eas_snn_amd
    eas_snn_amd.hip_library()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def golden():
    cases = split_cases(load_golden('cocoeval'))
    assert sorted(cases) == sorted(CASES)
    return cases


def _inputs(case, dev):
    return [torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in INPUTS]


def _run(case, dev, args=None, **kw):
    from eas_snn_amd import ops
    return ops.coco_eval(*(_inputs(case, dev) if args is None else args), int(case['num_images']), int(case['num_classes']), **kw)


@pytest.mark.parametrize('name', CASES)
def test_fixture_case_bit_for_bit(dev, golden, name):
    """precision and recall equal the reference binary's output (no tolerance), the non-ignored ground-truth counts equal the checker's"""
    case = golden[name]
    res = _run(case, dev)
    assert res['precision'].dtype == torch.float64 and res['precision'].shape == case['precision'].shape
    assert torch.equal(res['recall'].cpu(), torch.from_numpy(case['recall']))
    assert torch.equal(res['precision'].cpu(), torch.from_numpy(case['precision']))
    want = cocoeval_ref.evaluate(*[case[k] for k in INPUTS], case['num_images'], case['num_classes'])
    assert res['counts'].cpu().tolist() == want['counts'].tolist()


def test_gt_id_zero_is_the_only_id_that_matters(dev, golden):
    """the reference's quirk: with ids that start at 1 the detection matched to the first annotation becomes a true positive"""
    case = golden['thresholds']
    G = len(case['gt_box'])
    ids = torch.arange(1, G + 1, device=dev)
    res = _run(case, dev, gt_id=ids)
    want = cocoeval_ref.evaluate(*[case[k] for k in INPUTS], case['num_images'], case['num_classes'], gt_id=np.arange(1, G + 1))
    assert torch.equal(res['precision'].cpu(), torch.from_numpy(want['precision'])) and torch.equal(res['recall'].cpu(), torch.from_numpy(want['recall']))
    assert not np.array_equal(want['recall'], case['recall'])


def test_empty_inputs(dev, golden):
    """D = 0: curves of zeros where ground truth counts; G = 0 and both: all -1; zero images too.  Nothing faults."""
    from eas_snn_amd import ops
    case = golden['areas']
    no_det = dict(case, det_img=case['det_img'][:0], det_cls=case['det_cls'][:0], det_box=case['det_box'][:0], det_score=case['det_score'][:0])
    no_gt = dict(case, gt_img=case['gt_img'][:0], gt_cls=case['gt_cls'][:0], gt_box=case['gt_box'][:0])
    neither = dict(no_det, gt_img=case['gt_img'][:0], gt_cls=case['gt_cls'][:0], gt_box=case['gt_box'][:0])
    for c in (no_det, no_gt, neither, dict(neither, num_images=0)):
        res = _run(c, dev)
        want = cocoeval_ref.evaluate(*[c[k] for k in INPUTS], c['num_images'], c['num_classes'])
        assert torch.equal(res['precision'].cpu(), torch.from_numpy(want['precision']))
        assert torch.equal(res['recall'].cpu(), torch.from_numpy(want['recall']))
        assert res['counts'].cpu().tolist() == want['counts'].tolist()
    res = _run(no_det, dev)
    assert set(res['precision'].cpu().unique().tolist()) == {0.0} and set(res['recall'].cpu().unique().tolist()) == {0.0}
    assert set(_run(neither, dev)['precision'].cpu().unique().tolist()) == {-1.0}
    stats, lines = ops.coco_summarize(_run(neither, dev))
    assert stats.tolist() == [-1.0] * 12 and lines[0].endswith('= -1.000')


def test_twice_and_graph_replay_give_identical_bits(dev, golden):
    from eas_snn_amd import _lib
    case = golden['large']
    first, second = _run(case, dev), _run(case, dev)
    assert torch.equal(first['precision'], second['precision']) and torch.equal(first['recall'], second['recall'])
    args = _inputs(case, dev)
    side = _lib.private_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(case, dev, args, max_gt=8)                 # allocator warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            res = _run(case, dev, args, max_gt=8)       # (the caller states the ground truths per pair: no host synchronisation)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        res['precision'].fill_(7.0)
        res['recall'].fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(res['precision'], first['precision']) and torch.equal(res['recall'], first['recall'])
        assert torch.equal(res['counts'], first['counts'])


def test_beyond_a_limit_is_declined_without_a_launch(dev):
    """65 ground truths in one (image, category) (the limit is 64), and 17 IoU thresholds (16)"""
    from eas_snn_amd import _lib, ops
    lib = _lib.lib()
    box = torch.tensor([[0., 0., 10., 10.]], device=dev)
    z = torch.zeros(1, dtype=torch.int32, device=dev)
    many = (torch.zeros(65, dtype=torch.int32, device=dev), torch.zeros(65, dtype=torch.int32, device=dev), box.repeat(65, 1))
    before = lib.eas_launch_counter()
    assert not ops.coco_eval_supported(1, 65, 1, 1, max_gt=65) and ops.coco_eval_supported(1, 64, 1, 1, max_gt=64)
    with pytest.raises(_lib.EasHipError, match='limits'):
        ops.coco_eval(z, z, box, torch.ones(1, device=dev), *many, 1, 1)
    with pytest.raises(_lib.EasHipError, match='limits'):
        ops.coco_eval(z, z, box, torch.ones(1, device=dev), z, z, box, 1, 1, iou_thr=np.linspace(0.1, 0.9, 17))
    assert lib.eas_launch_counter() == before
    res = ops.coco_eval(z, z, box, torch.ones(1, device=dev), many[0][:64], many[1][:64], many[2][:64], 1, 1)       # 64 are fine
    assert res['counts'].cpu().tolist() == [[64, 64, 0, 0]]


def _records_to_arrays(records, labels_by_image):
    image_ids = sorted(labels_by_image)
    dense = {i: k for k, i in enumerate(image_ids)}
    det_img, det_cls, det_box, det_score = [], [], [], []
    for i, rec in records.items():
        b = np.array(rec['bboxes'], np.float32).reshape(-1, 4)
        b[:, 2:4] -= b[:, 0:2]                                    # xyxy -> xywh in float32, as convert_to_coco_format does
        det_box.append(b)
        det_img += [dense[i]] * len(b)
        det_cls += rec['categories']
        det_score += rec['scores']
    gt_img, gt_cls, gt_box = [], [], []
    for i, lab in labels_by_image.items():                         # loader order = annotation ids 0..
        for row in lab.tolist():
            gt_img.append(dense[i])
            gt_cls.append(int(row[4]))
            gt_box.append(row[:4])
    return (np.array(det_img), np.array(det_cls), np.concatenate(det_box), np.array(det_score, np.float32), np.array(gt_img), np.array(gt_cls),
            np.array(gt_box, np.float32), len(image_ids))


def test_evaluator_returns_the_checkers_ap(dev, tmp_path):
    """the set-up of test_evaluator_on_the_gpu (SYOLOX-S at 64x128, 10 samples, test_conf 0.00003): ap50_95 / ap50 equal the checker run on
    the returned image-wise records and the loader's labels to the last bit; the summary holds the twelve lines and both per-class tables;
    with ctx.device_ap off the fields are None and the old sentence is back"""
    from eas_snn_amd import ops
    from oracle import fill
    from yolox.exp import get_exp
    exp = get_exp(None, 'e-yolox-s')
    exp.merge(BASE_OPTS + ['use_spike', 'True', 'input_size', '(64, 128)', 'test_size', '(64, 128)', 'test_conf', '0.00003', 'nmsthre', '0.5'])
    exp.eval_samples, exp.eval_events, exp.eval_sensor_hw, exp.output_dir = 10, 3000, (60, 100), str(tmp_path)
    model = exp.get_model()
    fill.procedural_fill_(model, 2.0, ann_regex=fill.ANN_KEYS['True'])
    model.to(dev).eval()
    evaluator = exp.get_evaluator(2, False)
    assert ops.ctx.device_ap
    (ap50_95, ap50, summary), records = evaluator.evaluate(model, False, False, None, None, exp.test_size, return_outputs=True)
    assert isinstance(ap50_95, float) and isinstance(ap50, float) and 0.0 <= ap50_95 <= 1.0 and 0.0 <= ap50 <= 1.0
    labels = {}
    for _, labs, _, ids in evaluator.dataloader:
        labels.update({int(i): lab for i, lab in zip(ids, labs)})
    *arrays, n_images = _records_to_arrays(records, labels)
    assert len(arrays[0]) >= 20 and n_images == 10
    want = cocoeval_ref.evaluate(*arrays, n_images, 2)
    stats = cocoeval_ref.summarize(want['precision'], want['recall'])
    print(f'device AP {ap50_95!r} AP50 {ap50!r}; checker {stats[0]!r} {stats[1]!r}; {len(arrays[0])} detections')
    assert ap50_95 == stats[0] and ap50 == stats[1]
    assert torch.equal(evaluator.last_coco['precision'].cpu(), torch.from_numpy(want['precision']))
    assert torch.equal(evaluator.last_coco['recall'].cpu(), torch.from_numpy(want['recall']))
    assert evaluator.last_coco['counts'].cpu().tolist() == want['counts'].tolist()
    lines = [ln for ln in summary.split('\n') if ln.startswith(' Average ')]
    assert len(lines) == 12 and lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = {:0.3f}'.format(stats[0])
    assert lines[8] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = {:0.3f}'.format(stats[8])
    assert summary.startswith('Average forward time') and 'per class AP:\n| class' in summary and 'per class AR:\n| class' in summary
    # the distributed form of the feed (rank 0 uploads the gathered records) computes the same numbers
    data_list = [{'image_id': i, 'category_id': c, 'bbox': [b[0], b[1], float(np.float32(b[2]) - np.float32(b[0])), float(np.float32(b[3]) - np.float32(b[1]))],
                  'score': s, 'segmentation': []} for i, r in records.items() for b, s, c in zip(r['bboxes'], r['scores'], r['categories'])]
    gt_dict = {i: {'bboxes': lab[:, :4].tolist(), 'category_ids': [int(c) for c in lab[:, 4]]} for i, lab in labels.items()}
    up = evaluator.evaluate_prediction(data_list, gt_dict, evaluator.last_statistics, device=dev, feed=None)
    assert up[0] == ap50_95 and up[1] == ap50
    ops.ctx.device_ap = False
    try:
        (none_a, none_b, old), again = evaluator.evaluate(model, False, False, None, None, exp.test_size, return_outputs=True)
    finally:
        ops.ctx.device_ap = True
    assert again == records
    try:
        import pycocotools  # noqa: F401
    except ImportError:
        assert none_a is None and none_b is None and old.endswith('pycocotools is not installed: AP not computed\n')


def test_device_feed_equals_the_records(dev):
    """boxes and scores of the device feed carry the bits of convert_to_coco_format's records (scales that are no power of two)"""
    from yolox.evaluators import EventEvaluator
    ev = EventEvaluator(None, (64, 128), 0.01, 0.5, 2)
    g = torch.Generator().manual_seed(3)
    outputs = [torch.rand(37, 7, generator=g) * 100, None, torch.rand(5, 7, generator=g) * 100, torch.rand(64, 7, generator=g) * 100]
    for o in outputs:
        if o is not None:
            o[:, 2:4] += o[:, 0:2]
            o[:, 4:6] /= 100
            o[:, 6] = (o[:, 6] > 50).float()
    info = (torch.tensor([60, 60, 47, 33]), torch.tensor([100, 100, 131, 77]))
    ids = torch.tensor([11, 12, 5, 40])
    records = ev.convert_to_coco_format(outputs, info, ids)
    feed = []
    ev._feed_device_rows(feed, [None if o is None else o.to(dev) for o in outputs], info, ids, dev)
    (img, cls, box, score), = feed
    assert img.tolist() == [r['image_id'] for r in records] and cls.tolist() == [r['category_id'] for r in records]
    assert box.cpu().tolist() == [r['bbox'] for r in records] and score.cpu().tolist() == [r['score'] for r in records]


def test_evaluator_numbers_on_a_fixture_case(dev, golden):
    """evaluate_prediction fed the records of the 'large' case (image ids that are not dense): AP and AP50 of the reference binary's arrays"""
    from yolox.evaluators import EventEvaluator
    case = golden['large']
    loader = type('L', (), {'batch_size': 4, 'dataset': type('D', (), {'class_names': ['a', 'b']})()})()
    ev = EventEvaluator(loader, (256, 320), 0.01, 0.5, 2)
    image_id = lambda i: 3 + 7 * int(i)
    gt_dict = {image_id(i): {'bboxes': [], 'category_ids': []} for i in range(int(case['num_images']))}
    for i, c, b in zip(case['gt_img'], case['gt_cls'], case['gt_box']):
        gt_dict[image_id(i)]['bboxes'].append(b.tolist())
        gt_dict[image_id(i)]['category_ids'].append(int(c))
    order = np.argsort(case['gt_img'], kind='stable')              # the evaluator numbers annotations image by image
    assert np.array_equal(order, np.arange(len(order)))
    data = [{'image_id': image_id(i), 'category_id': int(c), 'bbox': b.tolist(), 'score': float(s), 'segmentation': []}
            for i, c, b, s in zip(case['det_img'], case['det_cls'], case['det_box'], case['det_score'])]
    ap, ap50, summary = ev.evaluate_prediction(data, gt_dict, torch.tensor([1.0, 1.0, 1.0]), device=dev)
    want = cocoeval_ref.summarize(case['precision'], case['recall'])
    assert ap == want[0] and ap50 == want[1] and 0.5 < ap < 0.52
    assert torch.equal(ev.last_coco['precision'].cpu(), torch.from_numpy(case['precision']))
    per_class = case['precision'][:, :, :, 0, -1]
    for k, name in enumerate('ab'):
        v = per_class[:, :, k]
        assert '| {} '.format(name) in summary and '{:.3f}'.format(float(np.mean(v[v > -1]) * 100)) in summary.split('per class AP:')[1]
