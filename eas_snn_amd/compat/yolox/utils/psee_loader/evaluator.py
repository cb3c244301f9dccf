"""Buffer of labels and predictions in front of ``evaluate_list`` (reference: yolox/utils/psee_loader/evaluator.py:11-79)."""
import warnings

import numpy as np

from .evaluation import evaluate_list


class PropheseeEvaluator:
    LABELS = 'lables'              # (the reference's spelling: the key is visible through ``_buffer``)
    PREDICTIONS = 'predictions'

    def __init__(self, dataset, downsample_by_2):
        assert dataset in {'gen1', 'gen4'}
        self.dataset = dataset
        self.downsample_by_2 = downsample_by_2
        self.reset_buffer()

    def _add(self, key, value):
        assert isinstance(value, list) and all(isinstance(v, np.ndarray) for v in value)
        self._buffer_empty = False
        self._buffer[key].extend(value)

    def add_predictions(self, predictions):
        self._add(self.PREDICTIONS, predictions)

    def add_labels(self, labels):
        self._add(self.LABELS, labels)

    def reset_buffer(self):
        self._buffer_empty = True
        self._buffer = {self.LABELS: [], self.PREDICTIONS: []}

    def has_data(self):
        return not self._buffer_empty

    def evaluate_buffer(self, img_height, img_width):
        """-> the six AP values over everything added since the last reset (None, with a warning, when nothing was added)"""
        if self._buffer_empty:
            warnings.warn('Attempt to use prophesee evaluation buffer, but it is empty', UserWarning, stacklevel=2)
            return None
        labels, predictions = self._buffer[self.LABELS], self._buffer[self.PREDICTIONS]
        assert len(labels) == len(predictions)
        return evaluate_list(result_boxes_list=predictions, gt_boxes_list=labels, height=img_height, width=img_width,
                             apply_bbox_filters=True, downsampled_by_2=self.downsample_by_2, camera=self.dataset)
