"""The box record of the Prophesee label files as a numpy structured type: eight little-endian fields packed from byte 0, the record padded
to 40 bytes (the layout the toolbox's .npy box files and the reference's evaluator use)."""
import numpy as np

_FIELDS = (('t', '<i8'), ('x', '<f4'), ('y', '<f4'), ('w', '<f4'), ('h', '<f4'), ('class_id', '<u4'), ('track_id', '<u4'),
           ('class_confidence', '<f4'))
RECORD_BYTES = 40


def _packed(fields, itemsize):
    offsets, at = [], 0
    for _, fmt in fields:
        offsets.append(at)
        at += np.dtype(fmt).itemsize
    assert at <= itemsize
    return np.dtype(dict(names=[n for n, _ in fields], formats=[f for _, f in fields], offsets=offsets, itemsize=itemsize))


BBOX_DTYPE = _packed(_FIELDS, RECORD_BYTES)
