"""``evaluate_list`` (reference: yolox/utils/psee_loader/evaluation.py:6-43): the camera's classes and thresholds, the filter on both
lists, then the matching and the COCO evaluation."""
from .io.box_filtering import filter_boxes
from .metrics.coco_eval import KEYS, boxes_to_device, device_route, evaluate_detection

CLASSES = {'gen1': ('car', 'pedestrian'), 'gen4': ('pedestrian', 'two-wheeler', 'car')}
SKIP_TS = int(5e5)


def thresholds(camera, downsampled_by_2=False):
    """(min_box_diag, min_box_side): 30 / 10 for gen1, 60 / 20 for gen4, integer-halved for recordings downsampled by 2"""
    assert camera in CLASSES
    diag, side = (60, 20) if camera == 'gen4' else (30, 10)
    return (diag // 2, side // 2) if downsampled_by_2 else (diag, side)


def evaluate_list(result_boxes_list, gt_boxes_list, height, width, camera='gen1', apply_bbox_filters=True, downsampled_by_2=False,
                  return_aps=True):
    """detections and ground truths as lists of structured arrays (one per file) -> the six AP values of the Prophesee protocol"""
    assert camera in CLASSES
    result_boxes_list, gt_boxes_list = list(result_boxes_list), list(gt_boxes_list)
    dev = device_route()
    if dev is not None:
        from eas_snn_amd import ops
        out, _ = ops.psee_eval(boxes_to_device(gt_boxes_list, dev, False), boxes_to_device(result_boxes_list, dev, True), camera=camera,
                               downsampled_by_2=downsampled_by_2, apply_bbox_filters=apply_bbox_filters)
        return out
    if apply_bbox_filters:
        diag, side = thresholds(camera, downsampled_by_2)
        gt_boxes_list = [filter_boxes(b, SKIP_TS, diag, side) for b in gt_boxes_list]
        result_boxes_list = [filter_boxes(b, SKIP_TS, diag, side) for b in result_boxes_list]
    return evaluate_detection(gt_boxes_list, result_boxes_list, height=height, width=width, classes=CLASSES[camera])


__all__ = ['evaluate_list', 'thresholds', 'CLASSES', 'KEYS']
