"""Evaluation under the Prophesee protocol (reference: yolox/evaluators/psee_evaluator.py:86-307, what ``tools/eval_event.py --eval_proh``
selects for the gen* datasets): EventEvaluator's inference loop -- graph replays, the two timers, frozen weights, the statistics triple --
with every sample as one "file" whose label time is read from its name, and ``evaluate_list`` of yolox/utils/psee_loader as the metric.

In a single process with the model on the GPU the rows of the post-processing never leave the device: they are turned into (t, xywh, class,
score) by the expressions of ``convert_to_gt_format`` there and handed to ``ops.psee_eval`` (filter -> time matching -> COCO evaluation, all
kernels).  With ``distributed=True`` rank 0 uploads the gathered structured arrays (``PropheseeEvaluator.evaluate_buffer``); a model on
the CPU or ``EAS_DEVICE_AP=0`` takes the numpy route of yolox/utils/psee_loader.

``evaluate`` returns ``(AP, AP_50, info)`` (and the predictions with ``return_outputs``); the reference returns ``('', info)`` without
``return_outputs``, which ``*_, summary = ...`` of tools/eval_event.py:209 reads the same way.  ``info`` is the timing line followed by one
line ``PROHESEE Evaluation/<key>  tensor(<value>)`` per result."""
import itertools

import numpy as np
import torch

from yolox.utils import gather, is_main_process, synchronize
from yolox.utils.psee_loader.evaluator import PropheseeEvaluator
from yolox.utils.psee_loader.records import BBOX_DTYPE
from yolox.utils.psee_loader.metrics.coco_eval import KEYS, NOT_COMPUTED

from .event_evaluator import EventEvaluator

__all__ = ['PSEEEvaluator', 'time_from_name']


def time_from_name(name):
    """label time in microseconds of a sample name ``<recording>a<time>`` (reference: get_time_from_name, :285-286)"""
    return int(str(name).split('a')[-1])


class PSEEEvaluator(EventEvaluator):
    """reference: yolox/evaluators/psee_evaluator.py:91-125 (same arguments)."""

    def __init__(self, dataloader, img_size, confthre, nmsthre, num_classes, testdev=False, per_class_AP=True, per_class_AR=True,
                 dataset='gen1', downsample_by_2=False, snn_reset=False):
        super().__init__(dataloader, img_size, confthre, nmsthre, num_classes, testdev, per_class_AP, per_class_AR, snn_reset)
        self.evaluator = PropheseeEvaluator(str(dataset).lower(), downsample_by_2)
        self.last_results = None            # the six values of the last evaluation
        self.last_match = None              # device route: sizes of the matched problem (images, detections, ground_truths)

    get_time_from_name = staticmethod(time_from_name)

    # ------------------------------------------------------------------ the loop
    def _evaluate_loop(self, model, distributed, decoder, return_outputs, dev, graph_ok):
        from eas_snn_amd._ctx import ctx
        device_ap = dev.type == 'cuda' and ctx.device_ap
        feed = [] if device_ap and not distributed else None          # single process: the rows stay on the device for the metric
        times = [0.0, 0.0]
        n_samples = max(len(self.dataloader) - 1, 1)
        self.evaluator.reset_buffer()
        names_of = self.dataloader.dataset.sample_names
        for outputs, labels, info_imgs, ids in self._run_batches(model, decoder, dev, graph_ok, times):
            sample_names = [names_of[int(i)] for i in ids]
            labels = [torch.as_tensor(label) for label in labels]
            if feed is not None and sample_names:                     # (an empty batch, the padding of a sharded evaluation, has no rows)
                self._feed_device_rows(feed, outputs, labels, info_imgs, sample_names, dev)
            batch_preds = self.convert_to_prophesee_format(self.convert_to_gt_format(outputs, info_imgs), sample_names)
            batch_labels = self.convert_to_prophesee_format([torch.cat([label, torch.ones_like(label[:, 0:1])], dim=1) for label in labels],
                                                            sample_names)
            if distributed:
                batch_preds = list(itertools.chain(*gather(batch_preds, dst=0)))
                batch_labels = list(itertools.chain(*gather(batch_labels, dst=0)))
            self.evaluator.add_labels(batch_labels)
            self.evaluator.add_predictions(batch_preds)
        statistics = torch.tensor([times[0], times[1], n_samples], dtype=torch.float32, device=dev)
        if distributed:
            synchronize()
            torch.distributed.reduce(statistics, dst=0)
        self.last_statistics = statistics
        eval_results = self.evaluate_prediction(statistics, device=dev if device_ap else None, feed=feed)
        predictions = self.evaluator._buffer[self.evaluator.PREDICTIONS]
        self.evaluator.reset_buffer()
        synchronize()
        if return_outputs:
            return eval_results, predictions
        return eval_results

    # ------------------------------------------------------------------ detections -> Prophesee records (:263-307)
    def _scale(self, img_h, img_w):
        return min(self.img_size[0] / float(img_h), self.img_size[1] / float(img_w))

    def convert_to_gt_format(self, outputs, info_imgs):
        """rows (x1, y1, x2, y2, obj, cls_conf, cls) per image -> [n, 6] (x, y, w, h, cls, score) on the raw sensor; an image without
        detections contributes the single all-zero row (the filter removes it).  The outputs are left untouched."""
        data_list = []
        for output, img_h, img_w in zip(outputs, info_imgs[0], info_imgs[1]):
            if output is None:
                data_list.append(torch.zeros((1, 6)))
                continue
            output = output.detach().cpu()
            bboxes = output[:, 0:4] / self._scale(img_h, img_w)
            bboxes[:, 2:4] -= bboxes[:, 0:2]
            data_list.append(torch.cat([bboxes, output[:, 6:7], (output[:, 4] * output[:, 5])[:, None]], dim=1))
        return data_list

    def convert_to_prophesee_format(self, bboxes, sample_names):
        """[n, 6] rows per sample -> structured arrays of the 40-byte box record, t = the sample's label time"""
        out = []
        for box, name in zip(bboxes, sample_names):
            box = np.asarray(box, np.float32).reshape(-1, 6)
            rec = np.zeros((len(box),), dtype=BBOX_DTYPE)
            rec['t'] = self.get_time_from_name(name)
            for j, k in enumerate('xywh'):
                rec[k] = box[:, j]
            rec['class_id'] = box[:, 4].astype(np.uint32)
            rec['class_confidence'] = box[:, 5]
            out.append(rec)
        return out

    def _feed_device_rows(self, feed, outputs, labels, info_imgs, sample_names, dev):
        """the batch for ``ops.psee_match`` without leaving the device: per sample (= file) its detections by the expressions of
        ``convert_to_gt_format`` (the division is by a tensor holding the float32 scale: a true division like the CPU's) and its labels;
        appends (times [B], det counts [B], det xywh, det class, det score, label counts [B], label xywh, label class)"""
        B = len(outputs)
        rows = torch.cat([torch.zeros((1, 7), dtype=torch.float32, device=dev) if o is None else o.detach() for o in outputs])
        counts = torch.tensor([1 if o is None else o.shape[0] for o in outputs], dtype=torch.int64)
        per_row = torch.repeat_interleave(torch.arange(B, device=dev), counts.to(dev), output_size=int(counts.sum()))
        scale = torch.tensor([self._scale(info_imgs[0][k], info_imgs[1][k]) for k in range(B)], dtype=torch.float32, device=dev)[per_row]
        xywh = rows[:, 0:4] / scale[:, None]
        xywh[:, 2:4] -= xywh[:, 0:2]
        lab = torch.cat(labels).to(dev, torch.float32).reshape(-1, 5)
        feed.append((torch.tensor([self.get_time_from_name(n) for n in sample_names], dtype=torch.int64), counts, xywh,
                     rows[:, 6].to(torch.int32), rows[:, 4] * rows[:, 5], torch.tensor([len(l) for l in labels], dtype=torch.int64),
                     lab[:, 0:4].contiguous(), lab[:, 4].to(torch.int32)))

    @staticmethod
    def _box_sets(feed, dev):
        """the batches' rows as the two box sets of ``ops.psee_match``: every sample is its own file"""
        times = torch.cat([f[0] for f in feed])

        def offsets(counts):
            return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)]).to(dev)
        d_counts, g_counts = torch.cat([f[1] for f in feed]), torch.cat([f[5] for f in feed])
        d_t, g_t = torch.repeat_interleave(times, d_counts).to(dev), torch.repeat_interleave(times, g_counts).to(dev)
        gt = (g_t, torch.cat([f[6] for f in feed]), torch.cat([f[7] for f in feed]), offsets(g_counts))
        dt = (d_t, torch.cat([f[2] for f in feed]), torch.cat([f[3] for f in feed]), torch.cat([f[4] for f in feed]), offsets(d_counts))
        return gt, dt

    # ------------------------------------------------------------------ summary (:238-261)
    def evaluate_prediction(self, statistics, device=None, feed=None):
        """-> (AP, AP_50, info).  ``feed``: the rows as device arrays (``_feed_device_rows``), evaluated by ``ops.psee_eval`` on ``device``;
        else the buffered records go through ``PropheseeEvaluator.evaluate_buffer``"""
        if not is_main_process():
            return 0, 0, None
        info = self._timing_line(statistics)
        if not self.evaluator.has_data():
            return 0, 0, info
        self.last_match = None
        if feed is not None and device is not None:
            from eas_snn_amd import ops
            gt, dt = self._box_sets(feed, device)
            results, res = ops.psee_eval(gt, dt, camera=self.evaluator.dataset, downsampled_by_2=self.evaluator.downsample_by_2)
            self.last_coco = res
            self.last_match = {k: res[k] for k in ('images', 'detections', 'ground_truths')}
        else:
            ds = getattr(self.dataloader, 'dataset', None)
            h, w = getattr(ds, 'img_size', None) or self.img_size
            results = self.evaluator.evaluate_buffer(h, w)
        self.last_results = results
        if results['AP'] is None:
            return None, None, info + NOT_COMPUTED + '\n'
        for k in KEYS:
            info += f'PROHESEE Evaluation/{k}  ' + str(torch.tensor(results[k])) + ' \n'
        return results['AP'], results['AP_50'], info
