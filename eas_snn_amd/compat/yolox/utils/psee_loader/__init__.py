"""Prophesee-protocol evaluation (reference: yolox/utils/psee_loader/{evaluation.py, evaluator.py, io/box_filtering.py, metrics/coco_eval.py}):
the box filter, the matching of detections to labelled timestamps and the COCO evaluation over the resulting images.  With a GPU the
whole chain runs on the device (``ops.psee_eval``); without one, or with ``EAS_DEVICE_AP=0``, filter and matching run in numpy."""
