"""The box filter of the Prophesee protocol (reference: yolox/utils/psee_loader/io/box_filtering.py:23-41), host form; the device form is
the mark stage of ``ops.psee_match`` (csrc/psee.hip)."""
import numpy as np


def keep_mask(t, w, h, skip_ts=int(5e5), min_box_diag=60, min_box_side=20):
    """rows later than ``skip_ts`` (strictly) whose squared diagonal, width and height reach the thresholds (inclusive).  float32
    arithmetic: each square and their sum are rounded on their own; the thresholds are compared as float32 values"""
    w, h = np.asarray(w, np.float32), np.asarray(h, np.float32)
    diag2 = np.add(np.multiply(w, w), np.multiply(h, h))
    late = np.asarray(t, np.int64) > int(skip_ts)
    return late & (diag2 >= np.float32(int(min_box_diag) ** 2)) & (w >= np.float32(min_box_side)) & (h >= np.float32(min_box_side))


def filter_boxes(boxes, skip_ts=int(5e5), min_box_diag=60, min_box_side=20):
    """structured box array (fields t, w, h among others) -> the rows the protocol evaluates (the defaults are the 1 Mpx camera's)"""
    return boxes[keep_mask(boxes['t'], boxes['w'], boxes['h'], skip_ts, min_box_diag, min_box_side)]
