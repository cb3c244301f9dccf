"""Matching of detections to labelled timestamps and the COCO evaluation over the resulting images (reference:
yolox/utils/psee_loader/metrics/coco_eval.py:25-179).  ``match_rows`` is the host form of ``ops.psee_match``: the same flat rows, in numpy."""
import numpy as np

KEYS = ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L')
NOT_COMPUTED = 'pycocotools is not installed: AP not computed'


def match_rows(gt_boxes_list, dt_boxes_list, time_tol=50000):
    """per file (the lists are parallel, rows ascending in t) one image per distinct ground-truth timestamp, in ascending order: its ground
    truths are the rows with that t, its detections the file's rows with ts - tol <= t <= ts + tol (so a detection can enter several
    images, and a file without ground truth yields none).  -> dict of flat arrays: gt_img / gt_cls int32, gt_box float32 [G,4], gt_id int64
    = 1..G, det_img / det_cls int32, det_box, det_score, image_file int32 [I], image_t int64 [I], num_images"""
    gi, gc, gb, di, dc, db, ds, image_file, image_t = [], [], [], [], [], [], [], [], []

    def xywh(a):
        return np.stack([a['x'], a['y'], a['w'], a['h']], 1).astype(np.float32).reshape(-1, 4)
    for f, (gt, dt) in enumerate(zip(gt_boxes_list, dt_boxes_list)):
        gt_t, dt_t = np.asarray(gt['t'], np.int64), np.asarray(dt['t'], np.int64)
        assert np.all(gt_t[1:] >= gt_t[:-1]) and np.all(dt_t[1:] >= dt_t[:-1]), 'the rows of a file must ascend in t'
        stamps = np.unique(gt_t)
        g0, g1 = np.searchsorted(gt_t, stamps, 'left'), np.searchsorted(gt_t, stamps, 'right')
        d0, d1 = np.searchsorted(dt_t, stamps - int(time_tol), 'left'), np.searchsorted(dt_t, stamps + int(time_tol), 'right')
        for k, ts in enumerate(stamps):
            i = len(image_t)
            image_file.append(f)
            image_t.append(int(ts))
            g, d = gt[g0[k]:g1[k]], dt[d0[k]:d1[k]]
            gi.append(np.full(len(g), i, np.int32))
            gc.append(g['class_id'].astype(np.int32))
            gb.append(xywh(g))
            di.append(np.full(len(d), i, np.int32))
            dc.append(d['class_id'].astype(np.int32))
            db.append(xywh(d))
            ds.append(d['class_confidence'].astype(np.float32))

    def cat(parts, dtype, tail=()):
        return np.concatenate(parts) if parts else np.zeros((0,) + tail, dtype)
    rows = dict(gt_img=cat(gi, np.int32), gt_cls=cat(gc, np.int32), gt_box=cat(gb, np.float32, (4,)), det_img=cat(di, np.int32),
                det_cls=cat(dc, np.int32), det_box=cat(db, np.float32, (4,)), det_score=cat(ds, np.float32),
                image_file=np.array(image_file, np.int32), image_t=np.array(image_t, np.int64), num_images=len(image_t))
    rows['gt_id'] = np.arange(1, len(rows['gt_img']) + 1, dtype=np.int64)
    return rows


def boxes_to_device(boxes_list, device, with_score):
    """list of structured arrays (one per file) -> the box set ``ops.psee_match`` takes, uploaded"""
    import torch
    boxes_list = list(boxes_list)
    n = [len(b) for b in boxes_list]
    offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)

    def field(name, dtype):
        return torch.from_numpy(np.concatenate([np.asarray(b[name]).astype(dtype) for b in boxes_list]) if boxes_list
                                else np.zeros(0, dtype)).to(device)
    box = torch.stack([field(k, np.float32) for k in 'xywh'], 1) if sum(n) else torch.zeros((0, 4), dtype=torch.float32, device=device)
    head = (field('t', np.int64), box.contiguous(), field('class_id', np.int64).to(torch.int32))
    return head + ((field('class_confidence', np.float32),) if with_score else ()) + (torch.from_numpy(offsets).to(device),)


def device_route():
    """the device the evaluation runs on, or None for the host route (no GPU, or ``EAS_DEVICE_AP=0``)"""
    import torch
    from eas_snn_amd._ctx import ctx
    if ctx.device_ap and torch.cuda.is_available():
        return torch.device('cuda', torch.cuda.current_device())
    return None


def host_ap(rows, classes, height=240, width=304):
    """AP over matched rows with pycocotools (default parameters, all images) -> the six values, or None when it cannot be imported"""
    try:
        from pycocotools.coco import COCO
        from pycocotools.cocoeval import COCOeval
    except ImportError:
        return None
    import contextlib
    import io
    gt = COCO()
    gt.dataset = {'info': {}, 'licenses': [], 'type': 'instances',
                  'images': [{'id': i + 1, 'file_name': 'n.a', 'height': height, 'width': width} for i in range(rows['num_images'])],
                  'annotations': [{'id': int(n), 'image_id': int(i) + 1, 'category_id': int(c) + 1, 'bbox': [float(v) for v in b],
                                   'area': float(b[2] * b[3]), 'iscrowd': False}
                                  for n, i, c, b in zip(rows['gt_id'], rows['gt_img'], rows['gt_cls'], rows['gt_box'])],
                  'categories': [{'id': k + 1, 'name': name, 'supercategory': 'none'} for k, name in enumerate(classes)]}
    results = [{'image_id': int(i) + 1, 'category_id': int(c) + 1, 'score': float(s), 'bbox': [float(v) for v in b]}
               for i, c, s, b in zip(rows['det_img'], rows['det_cls'], rows['det_score'], rows['det_box'])]
    with contextlib.redirect_stdout(io.StringIO()):
        gt.createIndex()
        ev = COCOeval(gt, gt.loadRes(results) if results else COCO(), 'bbox')
        ev.params.imgIds = np.arange(1, rows['num_images'] + 1, dtype=int)
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
    return {k: float(ev.stats[j]) for j, k in enumerate(KEYS)}


def evaluate_detection(gt_boxes_list, dt_boxes_list, classes=('car', 'pedestrian'), height=240, width=304, time_tol=50000, return_aps=True):
    """-> {'AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L'} over the images the (already filtered) lists give.  On the device when there is
    one and the classes are a camera's (2: gen1, 3: gen4); else numpy matching and pycocotools, or None values when that is missing"""
    gt_boxes_list, dt_boxes_list = list(gt_boxes_list), list(dt_boxes_list)
    assert len(gt_boxes_list) == len(dt_boxes_list), 'one detection array per ground-truth array'
    dev = device_route()
    camera = {2: 'gen1', 3: 'gen4'}.get(len(classes))
    if dev is not None and camera is not None:
        from eas_snn_amd import ops
        out, _ = ops.psee_eval(boxes_to_device(gt_boxes_list, dev, False), boxes_to_device(dt_boxes_list, dev, True), camera=camera,
                               apply_bbox_filters=False, time_tol=time_tol)
        return out
    out = host_ap(match_rows(gt_boxes_list, dt_boxes_list, time_tol), classes, height, width)
    return {k: None for k in KEYS} if out is None else out
