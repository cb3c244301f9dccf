"""Detections: batch-wide post-processing (confidence mask + class-aware NMS), COCO-style average precision, SimOTA assignment, decode +
loss terms + gradient (reference: yolox/utils/boxes.py:33-77; yolox/layers/cocoeval/cocoeval.cpp; yolox/models/yolo_head.py get_losses /
get_assignments).

Part of the operator layer of ``eas_snn_amd.ops`` (split by kernel family; ``ops`` re-exports everything here, so ``ops.<name>`` keeps working)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .ops_core import _call, _dev, _f32c, _timer_add, _timer_mark


# ------------------------------------------------------------------------------------------------ detections
def postprocess_device(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, class_agnostic=False):
    """(rows [B, A, 7], counts int32 [B]) on the device, no host synchronisation (eas_postprocess)."""
    _dev(prediction)
    pred = _f32c(prediction)
    B, A, row = pred.shape
    if row != 5 + num_classes:
        raise ValueError(f'prediction rows have {row} columns, expected 5 + {num_classes}')
    L = _lib.lib()
    out = torch.empty((B, A, 7), dtype=torch.float32, device=pred.device)
    cnt = torch.empty(B, dtype=torch.int32, device=pred.device)
    ws = torch.empty(L.eas_postprocess_workspace_bytes(B, A), dtype=torch.uint8, device=pred.device)
    check(L.eas_postprocess(ptr(pred), B, A, int(num_classes), float(conf_thre), float(nms_thre), int(bool(class_agnostic)), ptr(out),
                            ptr(cnt), ptr(ws), stream()), 'eas_postprocess')
    return out, cnt


def postprocess(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, class_agnostic=False):
    """``yolox.utils.postprocess`` (boxes.py:33-77): list with one [n, 7] tensor per image (None where nothing is kept)."""
    out, cnt = postprocess_device(prediction, num_classes, conf_thre, nms_thre, class_agnostic)
    counts = cnt.tolist()                                   # the one host synchronisation: the result is a ragged python list
    return [out[i, :n] if n else None for i, n in enumerate(counts)]


# ------------------------------------------------------------------------------------------------ average precision
COCO_AREA_NAMES = ('all', 'small', 'medium', 'large')
_COCO_TABLES = {}


def coco_default_params():
    """pycocotools' Params('bbox') -- the same numpy expressions, so the tables are bit-equal to the ones the reference evaluates with"""
    return dict(iou_thr=np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
                rec_thr=np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
                area_rng=np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64),
                max_dets=(1, 10, 100))


def _coco_tables(device, iou_thr, rec_thr, area_rng, max_dets):
    """the parameter tables as host numpy arrays and on the device (uploaded once per distinct set and device)"""
    d = coco_default_params()
    iou_thr = np.ascontiguousarray(d['iou_thr'] if iou_thr is None else iou_thr, np.float64).reshape(-1)
    rec_thr = np.ascontiguousarray(d['rec_thr'] if rec_thr is None else rec_thr, np.float64).reshape(-1)
    area_rng = np.ascontiguousarray(d['area_rng'] if area_rng is None else area_rng, np.float64).reshape(-1, 2)
    max_dets = np.ascontiguousarray(sorted(int(v) for v in max_dets), np.int32)
    if rec_thr.size > 1 and not np.all(np.diff(rec_thr) >= 0):
        raise ValueError('rec_thr must be ascending')
    key = (str(device), iou_thr.tobytes(), rec_thr.tobytes(), area_rng.tobytes(), max_dets.tobytes())
    t = _COCO_TABLES.get(key)
    if t is None:
        if len(_COCO_TABLES) >= 16:
            _COCO_TABLES.clear()
        t = _COCO_TABLES[key] = tuple(torch.from_numpy(a).to(device) for a in (iou_thr, rec_thr, area_rng, max_dets))
    return (iou_thr, rec_thr, area_rng, max_dets), t


def coco_eval_supported(D, G, num_images, num_classes, T=10, R=101, A=4, M=3, max_gt=0):
    """the limits of the eas_cocoeval_* kernels (include/eas_hip.h): at most 64 ground truths per (image, category), T <= 16, A <= 8,
    A * T <= 64, R <= 128, M <= 8, images * classes <= 2^24"""
    return bool(_lib.lib().eas_cocoeval_supported(int(D), int(G), int(num_images), int(num_classes), int(T), int(R), int(A), int(M), int(max_gt)))


@torch.no_grad()
def coco_eval(det_img, det_cls, det_box, det_score, gt_img, gt_cls, gt_box, num_images, num_classes, gt_id=None, iou_thr=None, rec_thr=None,
              area_rng=None, max_dets=(1, 10, 100), max_gt=None):
    """COCO bbox evaluation on the device: ``COCOeval(gt, dt, 'bbox')`` ``.evaluate()`` + ``.accumulate()`` as the reference's native module
    computes them (yolox/layers/cocoeval/cocoeval.cpp), bit for bit.  -> dict(precision float64 [T,R,K,A,M], recall float64 [T,K,A,M],
    counts int32 [K,A] = ground truths not ignored per (category, area range), params = the host tables), tensors on the device.

    det_img / gt_img: dense image index 0..num_images-1 (the position of the image id in the sorted ids); det_cls / gt_cls: 0..num_classes-1;
    boxes (x, y, w, h) float32; rows whose image or category is outside the tables are dropped, as pycocotools drops them.  Parameters
    default to pycocotools' (``coco_default_params``).  ``iscrowd`` is 0 throughout; the ``scores`` array is not produced.

    ``gt_id`` (default 0..G-1, the numbering of the reference's getcocoGT, event_evaluator.py:367) matters in one way, a quirk of the
    reference that is kept: a detection counts as matched when the id of its ground truth is not 0 (cocoeval.cpp:322-323, pycocotools'
    ``dtm``), so a detection matched to the annotation with id 0 takes that ground truth and still counts as unmatched.

    ``max_gt``: the largest number of ground truths in one (image, category) if the caller knows it; None computes it (one host
    synchronisation -- pass it under graph capture).  An input beyond the kernels' limits (``coco_eval_supported``) raises before anything
    is launched."""
    _dev(det_img, det_cls, det_box, det_score, gt_img, gt_cls, gt_box, gt_id)
    dev = det_box.device
    D, G, I, K = int(det_score.numel()), int(gt_img.numel()), int(num_images), int(num_classes)
    det_img, det_cls = det_img.to(torch.int32).contiguous(), det_cls.to(torch.int32).contiguous()
    gt_img, gt_cls = gt_img.to(torch.int32).contiguous(), gt_cls.to(torch.int32).contiguous()
    det_box, gt_box, det_score = _f32c(det_box).reshape(D, 4), _f32c(gt_box).reshape(G, 4), _f32c(det_score).reshape(D)
    gt_id = torch.arange(G, dtype=torch.int64, device=dev) if gt_id is None else gt_id.to(torch.int64).contiguous()
    host, (d_iou, d_rec, d_area, d_maxdets) = _coco_tables(dev, iou_thr, rec_thr, area_rng, max_dets)
    T, R, A, M = len(host[0]), len(host[1]), len(host[2]), len(host[3])
    if max_gt is None:
        max_gt = 0
        if G:
            ok = (gt_img >= 0) & (gt_img < I) & (gt_cls >= 0) & (gt_cls < K)
            counts = torch.unique((gt_img.long() * K + gt_cls)[ok], return_counts=True)[1]
            max_gt = int(counts.max()) if counts.numel() else 0
    L = _lib.lib()
    if not L.eas_cocoeval_supported(D, G, I, K, T, R, A, M, int(max_gt)):
        raise _lib.EasHipError(f'eas_cocoeval: beyond the kernels\' limits (D={D} G={G} images={I} classes={K} T={T} R={R} A={A} M={M}, '
                               f'{int(max_gt)} ground truths in one (image, category); include/eas_hip.h lists them)')
    i64 = dict(dtype=torch.int64, device=dev)
    det_key, gt_key = torch.empty(D, **i64), torch.empty(G, **i64)
    _call('eas_cocoeval_keys', 12 * D + 16 * G, L.eas_cocoeval_keys, ptr(det_img), ptr(det_cls), ptr(det_score), D, ptr(gt_img), ptr(gt_cls), G,
          I, K, ptr(det_key), ptr(gt_key), stream())
    det_key, det_order = torch.sort(det_key, stable=True)
    gt_key, gt_order = torch.sort(gt_key, stable=True)
    rank = torch.empty(D, dtype=torch.int32, device=dev)
    matched, ignored, key2 = torch.empty(D, **i64), torch.empty(D, **i64), torch.empty(D, **i64)
    npig = torch.empty((K, A), dtype=torch.int32, device=dev)
    _call('eas_cocoeval_match', 60 * D + 40 * G, L.eas_cocoeval_match, ptr(det_key), ptr(det_order), ptr(det_box), D, ptr(gt_key), ptr(gt_order),
          ptr(gt_box), ptr(gt_id), G, I, K, ptr(d_iou), T, ptr(d_area), A, int(host[3].max()) if M else 0, int(max_gt), ptr(rank), ptr(matched),
          ptr(ignored), ptr(key2), ptr(npig), stream())
    key2, order2 = torch.sort(key2, stable=True)
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
    ws = torch.empty(L.eas_cocoeval_workspace_bytes(D), dtype=torch.uint8, device=dev)
    _call('eas_cocoeval_accumulate', 48 * D + 20 * D * A * M + 8 * precision.numel(), L.eas_cocoeval_accumulate, ptr(key2),
          ptr(order2), ptr(rank), ptr(matched), ptr(ignored), D, ptr(npig), K, T, ptr(d_rec), R, A, ptr(d_maxdets), M, ptr(precision),
          ptr(recall), ptr(ws), stream())
    return dict(precision=precision, recall=recall, counts=npig,
                params=dict(iou_thr=host[0], rec_thr=host[1], area_rng=host[2], max_dets=[int(v) for v in host[3]]))


def coco_summarize(result):
    """``COCOeval.summarize`` for bbox (pycocotools cocoeval.py _summarizeDets): (stats float64 [12], the twelve text lines) from a
    ``coco_eval`` result.  stats = AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl, each the mean over the entries > -1 of
    its slice (-1 if there is none), taken on the host in float64 from the copied arrays."""
    precision, recall = result['precision'], result['recall']
    precision = precision.cpu().numpy() if torch.is_tensor(precision) else np.asarray(precision)
    recall = recall.cpu().numpy() if torch.is_tensor(recall) else np.asarray(recall)
    params = result.get('params') or coco_default_params()
    iou_thr, max_dets = np.asarray(params['iou_thr'], np.float64), [int(v) for v in params['max_dets']]
    if precision.shape[3] != len(COCO_AREA_NAMES) or len(max_dets) < 3:
        raise ValueError('coco_summarize needs the four area ranges (all, small, medium, large) and three max-dets entries')

    def one(ap, thr, area, md):
        a, m = COCO_AREA_NAMES.index(area), max_dets.index(md)
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == iou_thr)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        mean = float(np.mean(s[s > -1])) if len(s[s > -1]) else -1.0
        iou = '{:0.2f}:{:0.2f}'.format(iou_thr[0], iou_thr[-1]) if thr is None else '{:0.2f}'.format(thr)
        line = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
            'Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', iou, area, md, mean)
        return mean, line
    rows = [one(1, None, 'all', max_dets[2]), one(1, .5, 'all', max_dets[2]), one(1, .75, 'all', max_dets[2]),
            one(1, None, 'small', max_dets[2]), one(1, None, 'medium', max_dets[2]), one(1, None, 'large', max_dets[2]),
            one(0, None, 'all', max_dets[0]), one(0, None, 'all', max_dets[1]), one(0, None, 'all', max_dets[2]),
            one(0, None, 'small', max_dets[2]), one(0, None, 'medium', max_dets[2]), one(0, None, 'large', max_dets[2])]
    return np.array([r[0] for r in rows], np.float64), [r[1] for r in rows]



# ------------------------------------------------------------------------------------------------ Prophesee protocol
PSEE_CLASSES = {'gen1': ('car', 'pedestrian'), 'gen4': ('pedestrian', 'two-wheeler', 'car')}
PSEE_SKIP_TS = 500000
PSEE_KEYS = ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L')


def psee_thresholds(camera='gen1', downsampled_by_2=False):
    """(min_box_diag, min_box_side) of evaluate_list (yolox/utils/psee_loader/evaluation.py:24-35)"""
    if camera not in PSEE_CLASSES:
        raise ValueError(f"camera must be 'gen1' or 'gen4', got {camera!r}")
    diag, side = (60, 20) if camera == 'gen4' else (30, 10)
    return (diag // 2, side // 2) if downsampled_by_2 else (diag, side)


def _psee_set(s, with_score):
    """one box set as contiguous device arrays of the kernels' types: (t int64 [N], box fp32 [N,4], cls int32 [N], score fp32 [N] | None,
    file_offsets int64 [F+1])"""
    if len(s) != (5 if with_score else 4):
        raise ValueError('a box set is (t, box, cls, file_offsets) for ground truths and (t, box, cls, score, file_offsets) for detections')
    t, box, cls = s[0], s[1], s[2]
    score, off = (s[3], s[4]) if with_score else (None, s[3])
    _dev(t, box, cls, score, off)
    N = int(t.numel())
    t, cls, off = t.to(torch.int64).contiguous().reshape(N), cls.to(torch.int32).contiguous().reshape(-1), off.to(torch.int64).contiguous().reshape(-1)
    box = _f32c(box).reshape(-1, 4)
    score = _f32c(score).reshape(-1) if with_score else None
    if box.shape[0] != N or cls.numel() != N or (with_score and score.numel() != N) or off.numel() < 1:
        raise ValueError('the arrays of a box set must have one entry per row, and file_offsets F + 1 entries')
    return t, box, cls, score, off


def _scan(flags, exclusive):
    """int64 prefix sum of int32 flags: inclusive [N], or exclusive with the total appended [N + 1]"""
    if not exclusive:
        return torch.cumsum(flags, 0, dtype=torch.int64)
    out = torch.zeros(flags.numel() + 1, dtype=torch.int64, device=flags.device)
    torch.cumsum(flags, 0, dtype=torch.int64, out=out[1:])
    return out


@torch.no_grad()
def psee_match(gt, dt, camera='gen1', downsampled_by_2=False, apply_bbox_filters=True, time_tol=50000, sizes=None):
    """The Prophesee protocol in front of the COCO evaluation (``evaluate_list`` -> ``filter_boxes`` -> ``evaluate_detection`` /
    ``_match_times`` -> ``_to_coco_format`` of yolox/utils/psee_loader), on the device (the eas_psee kernels).  ``gt`` = (t, box, cls,
    file_offsets), ``dt`` = (t, box, cls, score, file_offsets): t int64 microseconds, box (x, y, w, h) float32, cls the 0-based class id;
    the rows of file f are [file_offsets[f], file_offsets[f + 1]) and ascend in t; both sets list the same files.

    Boxes of the first 0.5 s and boxes below the camera's size thresholds leave both sets (``apply_bbox_filters``); every distinct
    timestamp of a file's remaining ground truths is one image, numbered over the files in order, then by time; its detections are the
    file's remaining detections within +-``time_tol`` of it, both ends included -- a detection is copied into every image whose window
    holds it, and detections of a file without remaining ground truth disappear.

    -> dict: the arguments of ``ops.coco_eval`` (det_img int32 [D], det_cls int32, det_box, det_score, gt_img int32 [G], gt_cls, gt_box,
    gt_id = 1..G int64; rows image-major, inside an image in file row order), num_images, num_classes (from the camera), image_file
    int32 [I], image_t int64 [I], max_gt (the most ground truths in one (image, class)).

    The numbers only the device knows (images, detection rows, ground truths, max_gt) are read once in the middle: one host
    synchronisation.  ``sizes`` = (num_images, D, G, max_gt) of an earlier call on inputs of the same content skips the read (graph
    capture)."""
    g_t, g_box, g_cls, _, g_off = _psee_set(gt, False)
    d_t, d_box, d_cls, d_score, d_off = _psee_set(dt, True)
    if g_off.numel() != d_off.numel():
        raise ValueError(f'ground truths list {g_off.numel() - 1} files, detections {d_off.numel() - 1}')
    min_diag, min_side = psee_thresholds(camera, downsampled_by_2)
    K = len(PSEE_CLASSES[camera])
    dev = g_box.device
    Ng, Nd, F = int(g_t.numel()), int(d_t.numel()), int(g_off.numel()) - 1
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)

    def result(I, D, G, max_gt, rows=None, image_file=None, image_t=None):
        if rows is None:
            rows = (torch.empty(0, **i32), torch.empty(0, **i32), torch.empty((0, 4), dtype=torch.float32, device=dev), torch.empty(0, **i64),
                    torch.empty(0, **i32), torch.empty(0, **i32), torch.empty((0, 4), dtype=torch.float32, device=dev),
                    torch.empty(0, dtype=torch.float32, device=dev))
        return dict(gt_img=rows[0], gt_cls=rows[1], gt_box=rows[2], gt_id=rows[3], det_img=rows[4], det_cls=rows[5], det_box=rows[6],
                    det_score=rows[7], num_images=I, num_classes=K, max_gt=max_gt,
                    image_file=torch.empty(0, **i32) if image_file is None else image_file[:I],
                    image_t=torch.empty(0, **i64) if image_t is None else image_t[:I])
    if Ng == 0 or F == 0:
        return result(0, 0, 0, 0)
    L = _lib.lib()
    filt = int(bool(apply_bbox_filters))
    g_keep, g_first, d_keep = torch.empty(Ng, **i32), torch.empty(Ng, **i32), torch.empty(Nd, **i32)
    _call('eas_psee_mark', 32 * Ng, L.eas_psee_mark, ptr(g_t), ptr(g_box), Ng, ptr(g_off), F, PSEE_SKIP_TS, min_diag, min_side, filt,
          ptr(g_keep), ptr(g_first), stream())
    if Nd:
        _call('eas_psee_mark', 28 * Nd, L.eas_psee_mark, ptr(d_t), ptr(d_box), Nd, ptr(d_off), F, PSEE_SKIP_TS, min_diag, min_side, filt,
              ptr(d_keep), None, stream())
    g_keep_scan, g_img_scan, d_keep_scan = _scan(g_keep, True), _scan(g_first, False), _scan(d_keep, True)
    image_file, image_t = torch.empty(Ng, **i32), torch.empty(Ng, **i64)
    win_lo, win_cnt, pair_count = torch.empty(Ng, **i64), torch.empty(Ng, **i64), torch.empty((Ng, K), **i32)
    _call('eas_psee_windows', 60 * Ng, L.eas_psee_windows, ptr(g_t), ptr(g_cls), ptr(g_keep), ptr(g_first), ptr(g_img_scan), Ng, ptr(g_off),
          ptr(d_t), ptr(d_off), ptr(d_keep_scan), Nd, F, int(time_tol), K, ptr(image_file), ptr(image_t), ptr(win_lo), ptr(win_cnt),
          ptr(pair_count), stream())
    det_off = _scan(win_cnt, True)
    if sizes is None:
        # the one read: images, expanded detection rows, kept ground truths, the most ground truths in one (image, class)
        I, D, G, max_gt = torch.stack((g_img_scan[-1], det_off[-1], g_keep_scan[-1], pair_count.max().to(torch.int64))).tolist()
    else:
        I, D, G, max_gt = (int(v) for v in sizes)
    if I == 0:
        return result(0, 0, 0, 0)
    rows = (torch.empty(G, **i32), torch.empty(G, **i32), torch.empty((G, 4), dtype=torch.float32, device=dev), torch.empty(G, **i64),
            torch.empty(D, **i32), torch.empty(D, **i32), torch.empty((D, 4), dtype=torch.float32, device=dev),
            torch.empty(D, dtype=torch.float32, device=dev))
    _call('eas_psee_expand', 40 * Ng + 60 * D, L.eas_psee_expand, ptr(g_keep), ptr(g_keep_scan), ptr(g_img_scan), ptr(g_cls), ptr(g_box), Ng, G,
          ptr(det_off), ptr(win_lo), I, ptr(d_keep_scan), ptr(d_cls), ptr(d_box), ptr(d_score), Nd, D, *(ptr(r) for r in rows), stream())
    return result(I, D, G, max_gt, rows, image_file, image_t)


@torch.no_grad()
def psee_eval(gt, dt, camera='gen1', downsampled_by_2=False, apply_bbox_filters=True, time_tol=50000):
    """``evaluate_list`` (yolox/utils/psee_loader/evaluation.py) on the device: ``psee_match``, then ``coco_eval`` with annotation ids
    1..G (as _to_coco_format numbers them: no annotation has the id 0 that never counts as a match) and pycocotools' default parameters,
    then ``coco_summarize``.  -> ({'AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L'} = stats[0:6], the ``coco_eval`` result with the
    ``psee_match`` sizes added).  No image (no ground truth survives the filter) gives -1.0 six times.  ``coco_eval_supported`` is asked
    with the matched sizes before any evaluation kernel is launched; a refusal raises with the numbers."""
    m = psee_match(gt, dt, camera, downsampled_by_2, apply_bbox_filters, time_tol)
    D, G, I, K, max_gt = int(m['det_score'].numel()), int(m['gt_img'].numel()), m['num_images'], m['num_classes'], m['max_gt']
    if not coco_eval_supported(D, G, I, K, max_gt=max_gt):
        raise _lib.EasHipError(f'psee_eval: the matched rows are beyond the limits of the eas_cocoeval kernels (D={D} G={G} images={I} '
                               f'classes={K}, {max_gt} ground truths in one (image, category); include/eas_hip.h lists them)')
    res = coco_eval(m['det_img'], m['det_cls'], m['det_box'], m['det_score'], m['gt_img'], m['gt_cls'], m['gt_box'], I, K, gt_id=m['gt_id'],
                    max_gt=max_gt)
    stats, lines = coco_summarize(res)
    res = dict(res, detections=D, ground_truths=G, images=I, lines=lines, stats=stats)
    return {k: float(stats[j]) for j, k in enumerate(PSEE_KEYS)}, res


def simota_supported(gt_valid, bbox_preds):
    return bbox_preds.is_cuda and bbox_preds.dtype == torch.float32 and gt_valid.shape[1] <= 255 and bbox_preds.shape[1] <= 12288


@torch.no_grad()
def simota_assign(grids, strides, gt_boxes, gt_cls, gt_valid, bbox_preds, obj_preds, cls_preds):
    """SimOTA assignment for the whole batch in one launch (eas_simota_assign): (fg bool [B,A], matched int64 [B,A],
    matched_iou float [B,A]) -- the outputs of YOLOXHead._assign."""
    _dev(grids, strides, gt_boxes, gt_cls, gt_valid, bbox_preds, obj_preds, cls_preds)
    B, A = bbox_preds.shape[:2]
    G, nc = gt_valid.shape[1], cls_preds.shape[-1]
    gr = _f32c(grids.reshape(-1, 2)[:A].float())
    st = _f32c(strides.reshape(-1)[:A].float())
    gb, gc = _f32c(gt_boxes.float()), _f32c(gt_cls.float())
    gv = gt_valid.to(torch.uint8).contiguous()
    bx, ob, cl = _f32c(bbox_preds.float()), _f32c(obj_preds.float().reshape(B, A)), _f32c(cls_preds.float())
    fg = torch.empty((B, A), dtype=torch.uint8, device=bx.device)
    matched = torch.empty((B, A), dtype=torch.int64, device=bx.device)
    miou = torch.empty((B, A), dtype=torch.float32, device=bx.device)
    check(_lib.lib().eas_simota_assign(ptr(gr), ptr(st), ptr(gb), ptr(gc), ptr(gv), ptr(bx), ptr(ob), ptr(cl), B, G, A, nc, ptr(fg),
                                       ptr(matched), ptr(miou), stream()), 'eas_simota_assign')
    return fg.bool(), matched, miou


_ANCHOR_CACHE = {}


def _anchor_tables(hws, strides, device):
    """grids [A,2] and strides [A] of the head levels (cached per geometry and device)"""
    key = (tuple(hws), tuple(float(s_) for s_ in strides), str(device))
    t = _ANCHOR_CACHE.get(key)
    if t is None:
        gs, ss = [], []
        for (h, w), s_ in zip(hws, strides):
            yv, xv = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
            gs.append(torch.stack((xv, yv), 2).reshape(-1, 2).float())
            ss.append(torch.full((h * w,), float(s_)))
        t = _ANCHOR_CACHE[key] = (torch.cat(gs).to(device), torch.cat(ss).to(device))
    return t


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _DetLossFn(torch.autograd.Function):
    """Decode + SimOTA assignment + loss terms + their gradient for the raw head maps of all levels: five launches forward
    (eas_det_decode, eas_simota_assign_rows, eas_det_loss x2) plus a few tiny label ops, one multiply backward."""

    @staticmethod
    def forward(ctx, labels, strides, nc, use_l1, *raw):
        ctx.set_materialize_grads(False)      # a result nobody differentiates arrives as None in backward, not as a zero tensor
        L = len(raw) // 3
        regs, objs, clss = [_f32c(t) for t in raw[0::3]], [_f32c(t) for t in raw[1::3]], [_f32c(t) for t in raw[2::3]]
        _dev(labels, *regs)
        lib = _lib.lib()
        dev = regs[0].device
        B = regs[0].shape[0]
        hws = [tuple(r.shape[-2:]) for r in regs]
        A = sum(h * w for h, w in hws)
        hw_arr = (C.c_int * (2 * L))(*[v for hw in hws for v in hw])
        st_arr = (C.c_float * L)(*[float(s_) for s_ in strides])
        dec = torch.empty((B, A, 5 + nc), dtype=torch.float32, device=dev)
        check(lib.eas_det_decode(L, _ptr_array(regs), _ptr_array(objs), _ptr_array(clss), hw_arr, st_arr, B, nc, ptr(dec), stream()),
              'eas_det_decode')
        labels = _f32c(labels.float())
        G = labels.shape[1]
        if B <= 1024 and labels.shape[2] == 5:
            # nlabel, the valid-row mask, class / box columns and the label count as ONE launch instead of ten tiny tensor operators
            gt_valid = torch.empty((B, G), dtype=torch.uint8, device=dev)
            gt_cls = torch.empty((B, G), dtype=torch.float32, device=dev)
            gt_boxes = torch.empty((B, G, 4), dtype=torch.float32, device=dev)
            num_gts = torch.empty((), dtype=torch.float32, device=dev)
            check(lib.eas_det_labels(ptr(labels), B, G, ptr(gt_valid), ptr(gt_cls), ptr(gt_boxes), ptr(num_gts), stream()), 'eas_det_labels')
        else:
            nlabel = (labels.sum(dim=2) > 0).sum(dim=1)
            gt_valid = (torch.arange(G, device=dev)[None] < nlabel[:, None]).to(torch.uint8)
            gt_cls, gt_boxes = labels[:, :, 0].contiguous(), labels[:, :, 1:5].contiguous()
            num_gts = nlabel.sum().float()
        grids, svec = _anchor_tables(hws, strides, dev)
        fg = torch.empty((B, A), dtype=torch.uint8, device=dev)
        matched = torch.empty((B, A), dtype=torch.int64, device=dev)
        miou = torch.empty((B, A), dtype=torch.float32, device=dev)
        check(lib.eas_simota_assign_rows(ptr(grids), ptr(svec), ptr(gt_boxes), ptr(gt_cls), ptr(gt_valid), ptr(dec), B, G, A, nc, ptr(fg),
                                         ptr(matched), ptr(miou), stream()), 'eas_simota_assign_rows')
        g_regs, g_objs, g_clss = [torch.empty_like(t) for t in regs], [torch.empty_like(t) for t in objs], [torch.empty_like(t) for t in clss]
        out = torch.empty(7, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.eas_det_loss_workspace_doubles(), dtype=torch.float64, device=dev)
        check(lib.eas_det_loss(L, _ptr_array(regs), _ptr_array(objs), _ptr_array(clss), _ptr_array(g_regs), _ptr_array(g_objs),
                               _ptr_array(g_clss), hw_arr, st_arr, B, nc, ptr(dec), ptr(gt_boxes), ptr(gt_cls), G, ptr(fg), ptr(matched),
                               ptr(miou), ptr(num_gts), int(bool(use_l1)), ptr(out), ptr(ws), stream()), 'eas_det_loss')
        ctx.grads = [g for trip in zip(g_regs, g_objs, g_clss) for g in trip]
        ctx.scale = out[6]
        outs = tuple(out[i] for i in range(6))
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    def backward(ctx, g_total, *_unused):
        grads = ctx.grads
        if g_total is None:
            return (None,) * (4 + len(grads))
        # out of place: ctx.grads keep d(total * num_fg)/d(raw), so a second backward through a retained graph scales the same maps again
        return (None, None, None, None) + tuple(torch._foreach_mul(grads, g_total * ctx.scale))


def det_decode_eval_supported(raws):
    return (len(raws) <= 4 and all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 for trip in raws for t in trip)
            and sum(r.shape[-1] * r.shape[-2] for r, _, _ in raws) < (1 << 24))


@torch.no_grad()
def det_decode_eval(raws, strides, num_classes):
    """inference output [B, A, 5 + num_classes] of YOLOXHead from the raw (reg, obj, cls) maps of its levels: sigmoid on objectness and
    classes, levels along the anchors, boxes decoded -- one launch (eas_det_decode_eval)."""
    regs, objs, clss = [_f32c(r) for r, _, _ in raws], [_f32c(o) for _, o, _ in raws], [_f32c(c) for _, _, c in raws]
    _dev(*regs)
    L = len(regs)
    B = regs[0].shape[0]
    hws = [tuple(r.shape[-2:]) for r in regs]
    A = sum(h * w for h, w in hws)
    hw_arr = (C.c_int * (2 * L))(*[v for hw in hws for v in hw])
    st_arr = (C.c_float * L)(*[float(s_) for s_ in strides])
    dec = torch.empty((B, A, 5 + num_classes), dtype=torch.float32, device=regs[0].device)
    _call('eas_det_decode', 4 * 2 * dec.numel(), _lib.lib().eas_det_decode_eval, L, _ptr_array(regs), _ptr_array(objs), _ptr_array(clss), hw_arr,
          st_arr, B, int(num_classes), ptr(dec), stream())
    return dec


def det_loss_supported(raw_regs, labels, loss_type):
    A = sum(r.shape[-1] * r.shape[-2] for r in raw_regs)
    return (raw_regs[0].is_cuda and raw_regs[0].dtype == torch.float32 and len(raw_regs) <= 4 and A <= 12288 and labels.shape[1] <= 255
            and loss_type == 'iou' and all(r.dim() == 4 for r in raw_regs))


def det_loss(regs, objs, clss, labels, strides, num_classes, use_l1):
    """(total, 5*iou, obj, cls, l1, num_fg/num_gts) of YOLOXHead.get_losses from the raw head maps of every level."""
    raw = [t for trip in zip(regs, objs, clss) for t in trip]
    return _DetLossFn.apply(labels, tuple(float(s_) for s_ in strides), int(num_classes), bool(use_l1), *raw)
