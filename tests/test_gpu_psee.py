"""GPU tests of the Prophesee-protocol evaluation on the device (``ops.psee_match`` / ``ops.psee_eval``, the eas_psee kernels in front of the
eas_cocoeval ones): every case of tests/golden/psee.npz -- rows recorded from the reference's filter and time matching, precision / recall
from its native COCO evaluation -- bit for bit; empty inputs; the filter switched off; determinism and graph replay; PSEEEvaluator end to end."""
import numpy as np
import pytest
import torch

from conftest import load_golden, split_cases

from test_cpu_psee import CASES, box_lists

pytestmark = pytest.mark.gpu

BASE_OPTS = ['T', '3', 'embedding', 'arsnn', 'num_classes', '2', 'spike_attach', 'True', 'thresh', '1', 'readout', 'sum',
             'embedding_depth', '2', 'embedding_ksize', '5', 'write_zero', 'True', 'spike_fn', 'atan']
ROWS = ('det_img', 'det_cls', 'det_box', 'det_score', 'gt_img', 'gt_cls', 'gt_box', 'gt_id', 'image_file', 'image_t')
KEYS = ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    import eas_snn_amd
    eas_snn_amd.hip_library()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def golden():
    cases = split_cases(load_golden('psee'))
    assert sorted(cases) == sorted(CASES)
    return cases


def _sets(case, dev):
    up = lambda k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev)
    return (tuple(up(k) for k in ('gt_t', 'gt_box', 'gt_cls', 'gt_offsets')),
            tuple(up(k) for k in ('dt_t', 'dt_box', 'dt_cls', 'dt_score', 'dt_offsets')))


def _kw(case):
    return dict(camera=str(case['camera']), downsampled_by_2=bool(case['downsampled_by_2']), time_tol=int(case['time_tol']))


def _assert_rows(m, case):
    assert m['num_images'] == int(case['num_images'])
    for k in ROWS:
        want = torch.from_numpy(case['out_' + k])
        assert m[k].dtype == want.dtype and m[k].shape == want.shape and torch.equal(m[k].cpu(), want), k


@pytest.mark.parametrize('name', CASES)
def test_match_rows_bit_for_bit(dev, golden, name):
    from eas_snn_amd import ops
    case = golden[name]
    m = ops.psee_match(*_sets(case, dev), **_kw(case))
    _assert_rows(m, case)
    pairs = np.bincount(case['out_gt_img'].astype(np.int64) * m['num_classes'] + case['out_gt_cls'])
    assert m['max_gt'] == int(pairs.max()) and m['num_classes'] == case['precision'].shape[2]


@pytest.mark.parametrize('name', CASES)
def test_eval_bit_for_bit(dev, golden, name):
    from eas_snn_amd import ops
    case = golden[name]
    out, res = ops.psee_eval(*_sets(case, dev), **_kw(case))
    assert torch.equal(res['recall'].cpu(), torch.from_numpy(case['recall']))
    assert torch.equal(res['precision'].cpu(), torch.from_numpy(case['precision']))
    assert list(out) == list(KEYS) and [out[k] for k in KEYS] == case['stats'].tolist()
    assert res['images'] == int(case['num_images']) and res['detections'] == len(case['out_det_img'])


def test_empty_inputs(dev, golden):
    """no files; files without rows; ground truths but no detections at all; everything filtered: no image, six times -1.0, no launch error"""
    from eas_snn_amd import ops
    case = golden['samples']
    gt, dt = _sets(case, dev)
    z64 = torch.zeros(1, dtype=torch.int64, device=dev)
    no_files = ((gt[0][:0], gt[1][:0], gt[2][:0], z64), (dt[0][:0], dt[1][:0], dt[2][:0], dt[3][:0], z64))
    no_rows = ((gt[0][:0], gt[1][:0], gt[2][:0], torch.zeros(5, dtype=torch.int64, device=dev)),
               (dt[0][:0], dt[1][:0], dt[2][:0], dt[3][:0], torch.zeros(5, dtype=torch.int64, device=dev)))
    early = ((gt[0] * 0 + 500000,) + gt[1:], (dt[0] * 0 + 500000,) + dt[1:])
    tiny = ((gt[0], gt[1] * 0 + 9.75) + gt[2:], dt)
    for sets in (no_files, no_rows, early, tiny):
        m = ops.psee_match(*sets)
        assert m['num_images'] == 0 and m['max_gt'] == 0 and all(m[k].numel() == 0 for k in ROWS)
        assert m['det_box'].shape == (0, 4) and m['gt_id'].dtype == torch.int64
        out, res = ops.psee_eval(*sets)
        assert [out[k] for k in KEYS] == [-1.0] * 6 and set(res['precision'].cpu().unique().tolist()) == {-1.0}
    # ground truths without a single detection row: images, and curves of zeros
    none = (dt[0][:0], dt[1][:0], dt[2][:0], dt[3][:0], torch.zeros_like(dt[4]))
    m = ops.psee_match(gt, none)
    assert m['num_images'] == int(case['num_images']) and m['det_img'].numel() == 0
    assert torch.equal(m['gt_box'].cpu(), torch.from_numpy(case['out_gt_box']))
    out, _ = ops.psee_eval(gt, none)
    assert out['AP'] == 0.0
    with pytest.raises(ValueError, match='files'):
        ops.psee_match(gt, no_files[1])
    torch.cuda.synchronize()


def test_filters_off(dev, golden):
    """apply_bbox_filters=False: every row takes part, the first 0.5 s included -- the host route's rows"""
    from eas_snn_amd import ops
    from yolox.utils.psee_loader.metrics.coco_eval import match_rows
    for name in ('filters_gen1', 'windows'):
        case = golden[name]
        gts, dts = box_lists(case)
        want = match_rows(gts, dts, int(case['time_tol']))
        m = ops.psee_match(*_sets(case, dev), apply_bbox_filters=False, **_kw(case))
        assert m['num_images'] == want['num_images'] > int(case['num_images']) and m['gt_img'].numel() == len(case['gt_t'])
        for k in ROWS:
            assert torch.equal(m[k].cpu(), torch.from_numpy(want[k])), k


def test_other_tolerance(dev, golden):
    """time_tol = 10 ms and 0: the host route's rows (windows no longer overlap; exact timestamps only)"""
    from eas_snn_amd import ops
    from test_cpu_psee import host_rows
    for tol in (10000, 0):
        case = dict(golden['windows'], time_tol=np.int64(tol))
        want, _ = host_rows(case)
        m = ops.psee_match(*_sets(case, dev), **_kw(case))
        for k in ROWS:
            assert torch.equal(m[k].cpu(), torch.from_numpy(want[k])), k


def test_twice_and_graph_replay_give_identical_bits(dev, golden):
    from eas_snn_amd import _lib, ops
    case = golden['large']
    sets, kw = _sets(case, dev), _kw(case)
    first, second = ops.psee_match(*sets, **kw), ops.psee_match(*sets, **kw)
    for k in ROWS:
        assert torch.equal(first[k], second[k]), k
    sizes = (first['num_images'], first['det_img'].numel(), first['gt_img'].numel(), first['max_gt'])       # the sizing read stays outside
    side = _lib.private_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.psee_match(*sets, sizes=sizes, **kw)            # allocator warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            m = ops.psee_match(*sets, sizes=sizes, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for k in ROWS:
            m[k].fill_(7)
        g.replay()
        torch.cuda.synchronize()
        for k in ROWS:
            assert torch.equal(m[k], first[k]), k
    _assert_rows(m, case)


def test_beyond_a_limit_raises_with_the_numbers(dev):
    """65 ground truths of one class on one timestamp: the evaluation kernels' limit is 64; nothing of theirs is launched"""
    from eas_snn_amd import _lib, ops
    box = torch.tensor([[10., 10., 40., 40.]], device=dev)
    off = torch.tensor([0, 65], device=dev)
    gt = (torch.full((65,), 600000, device=dev), box.repeat(65, 1), torch.zeros(65, dtype=torch.int32, device=dev), off)
    dt = (gt[0][:1], box, gt[2][:1], torch.ones(1, device=dev), torch.tensor([0, 1], device=dev))
    m = ops.psee_match(gt, dt)
    assert m['max_gt'] == 65 and m['num_images'] == 1 and m['gt_id'].tolist() == list(range(1, 66))
    with pytest.raises(_lib.EasHipError, match='65 ground truths in one'):
        ops.psee_eval(gt, dt)
    out, _ = ops.psee_eval(tuple(a[:64] for a in gt[:3]) + (torch.tensor([0, 64], device=dev),), dt)
    assert out['AP'] >= 0.0


def _exp(tmp_path):
    from yolox.exp import get_exp
    exp = get_exp(None, 'e-yolox-s')
    exp.merge(BASE_OPTS + ['use_spike', 'True', 'input_size', '(64, 96)', 'test_size', '(64, 96)', 'test_conf', '0.00003', 'nmsthre', '0.5',
                           'data_name', 'gen1', 'eval_proph', 'True'])
    exp.eval_samples, exp.eval_events, exp.eval_label_period_us, exp.output_dir = 8, 3000, 200000, str(tmp_path)
    return exp


def test_evaluator_end_to_end(dev, tmp_path, monkeypatch):
    """SYOLOX-S on a 64 x 96 canvas, 8 samples labelled 200 ms apart (the first three fall to the 0.5 s rule) in batches of 4: eager and
    graphed evaluations agree; the result equals the host route fed the evaluator's own gathered records; the single-process device feed
    equals the uploaded records"""
    from eas_snn_amd import ops
    from oracle import fill
    from yolox.evaluators import PSEEEvaluator
    from yolox.utils.psee_loader.evaluation import SKIP_TS, thresholds
    from yolox.utils.psee_loader.io.box_filtering import filter_boxes
    from yolox.utils.psee_loader.metrics.coco_eval import boxes_to_device, match_rows
    import cocoeval_ref
    exp = _exp(tmp_path)
    model = exp.get_model()
    fill.procedural_fill_(model, 2.0, ann_regex=fill.ANN_KEYS['True'])
    model.to(dev).eval()
    evaluator = exp.get_evaluator(2, False)
    assert type(evaluator) is PSEEEvaluator and evaluator.dataloader.batch_size == 4 and len(evaluator.dataloader) == 2
    (ap, ap50, info), preds = evaluator.evaluate(model, False, False, None, None, exp.test_size, return_outputs=True)
    assert evaluator.graphs_recorded == 1 and isinstance(ap, float) and 0.0 <= ap <= 1.0 and 0.0 <= ap50 <= 1.0
    print(f'{sum(len(p) for p in preds)} detection rows, matched problem {evaluator.last_match}')
    assert len(preds) == 8 and sum(len(p) for p in preds) > 8           # (8 rows would be placeholders alone)
    assert evaluator.last_match['images'] == 5 and evaluator.last_match['detections'] > 0
    lines = info.split('\n')
    assert lines[0].startswith('Average forward time') and lines[1] == 'PROHESEE Evaluation/AP  ' + str(torch.tensor(ap)) + ' '
    assert [ln.split('  ')[0] for ln in lines[1:7]] == ['PROHESEE Evaluation/' + k for k in KEYS]
    graphed = dict(evaluator.last_results)
    # eager
    monkeypatch.setenv('EAS_EVAL_GRAPH', '0')
    eager = exp.get_evaluator(2, False)
    (ap_e, ap50_e, _), preds_e = eager.evaluate(model, False, False, None, None, exp.test_size, return_outputs=True)
    # (the forward at this canvas is not bit-reproducible from one run to the next -- the last bit of a few boxes and scores moves, also
    # between two graph replays -- so runs are compared by their results and record counts; every bitwise comparison below stays inside
    # ONE evaluation: device against host on the same records)
    assert eager.graphs_recorded == 0 and eager.last_results == graphed and (ap_e, ap50_e) == (ap, ap50)
    assert [len(p) for p in preds_e] == [len(p) for p in preds] and eager.last_match['images'] == 5
    # the host route on the evaluator's own records: rows by numpy, AP by the checker
    labels = []
    for _, labs, _, ids in evaluator.dataloader:
        names = [evaluator.dataloader.dataset.sample_names[int(i)] for i in ids]
        labels += evaluator.convert_to_prophesee_format([torch.cat([lab, torch.ones_like(lab[:, :1])], 1) for lab in labs], names)
    diag, side = thresholds('gen1')
    rows = match_rows([filter_boxes(g, SKIP_TS, diag, side) for g in labels], [filter_boxes(d, SKIP_TS, diag, side) for d in preds])
    assert rows['num_images'] == 5 and rows['image_t'].tolist() == [600000, 800000, 1000000, 1200000, 1400000]
    want = cocoeval_ref.evaluate(*[rows[k] for k in ('det_img', 'det_cls', 'det_box', 'det_score', 'gt_img', 'gt_cls', 'gt_box')], 5, 2,
                                 gt_id=rows['gt_id'])
    stats = cocoeval_ref.summarize(want['precision'], want['recall'])
    print(f'device {graphed}; checker {stats[:6].tolist()}; {len(rows["det_img"])} matched detections')
    assert [graphed[k] for k in KEYS] == stats[:6].tolist()
    assert torch.equal(evaluator.last_coco['precision'].cpu(), torch.from_numpy(want['precision']))
    # the uploaded-records feed (what rank 0 of a distributed evaluation does) against the device feed
    m = ops.psee_match(boxes_to_device(labels, dev, False), boxes_to_device(preds, dev, True))
    for k in ROWS:
        assert torch.equal(m[k].cpu(), torch.from_numpy(rows[k])), k
    evaluator.evaluator.add_labels(labels)
    evaluator.evaluator.add_predictions(preds)
    assert evaluator.evaluator.evaluate_buffer(64, 96) == graphed
    up = evaluator.evaluate_prediction(evaluator.last_statistics, device=dev, feed=None)
    assert (up[0], up[1]) == (ap, ap50)
    evaluator.evaluator.reset_buffer()
    # EAS_DEVICE_AP=0: the numpy route; the records are the same
    ops.ctx.device_ap = False
    try:
        (a0, b0, old), again = evaluator.evaluate(model, False, False, None, None, exp.test_size, return_outputs=True)
    finally:
        ops.ctx.device_ap = True
    assert [len(p) for p in again] == [len(p) for p in preds]
    try:
        import pycocotools  # noqa: F401
    except ImportError:
        assert a0 is None and b0 is None and old.endswith('pycocotools is not installed: AP not computed\n')


def test_device_feed_equals_the_records(dev):
    """rows of the device feed carry the bits of convert_to_gt_format's records (scales that are no power of two; an image without
    detections gives the all-zero row in both)"""
    from yolox.evaluators import PSEEEvaluator
    ev = PSEEEvaluator(None, (64, 128), 0.01, 0.5, 2)
    g = torch.Generator().manual_seed(3)
    outputs = [torch.rand(37, 7, generator=g) * 100, None, torch.rand(5, 7, generator=g) * 100, torch.rand(64, 7, generator=g) * 100]
    for o in outputs:
        if o is not None:
            o[:, 2:4] += o[:, 0:2]
            o[:, 4:6] /= 100
            o[:, 6] = (o[:, 6] > 50).float()
    info = (torch.tensor([60, 60, 47, 33]), torch.tensor([100, 100, 131, 77]))
    names = ['ra700000', 'ra800000', 'ra900000', 'ra5000000000']
    labels = [torch.tensor([[1., 2., 30., 40., 1.]]), torch.zeros((0, 5)), torch.tensor([[5., 6., 7., 8., 0.], [9., 10., 11., 12., 1.]]),
              torch.tensor([[3., 4., 50., 60., 0.]])]
    recs = ev.convert_to_prophesee_format(ev.convert_to_gt_format(outputs, info), names)
    feed = []
    ev._feed_device_rows(feed, [None if o is None else o.to(dev) for o in outputs], labels, info, names, dev)
    gt, dt = ev._box_sets(feed, dev)
    cat = np.concatenate(recs)
    assert dt[0].tolist() == cat['t'].tolist() and dt[4].tolist() == [0, 37, 38, 43, 107]
    assert dt[1].cpu().tolist() == np.stack([cat[k] for k in 'xywh'], 1).tolist()
    assert dt[2].tolist() == cat['class_id'].tolist() and dt[3].cpu().tolist() == cat['class_confidence'].tolist()
    assert gt[3].tolist() == [0, 1, 1, 3, 4] and gt[0].tolist() == [700000, 900000, 900000, 5000000000]
    assert gt[1].cpu().tolist() == [[1., 2., 30., 40.], [5., 6., 7., 8.], [9., 10., 11., 12.], [3., 4., 50., 60.]] and gt[2].tolist() == [1, 0, 1, 0]
