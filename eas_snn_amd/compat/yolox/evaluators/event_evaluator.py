"""Inference loop of the evaluation side of the boundary (reference: yolox/evaluators/event_evaluator.py:83-263, the part that
``tools/eval_event.py:209-211`` and ``Trainer.evaluate_and_save_model`` call).

What is kept: the constructor and ``evaluate`` signatures, per batch forward -> ``reset_net`` -> (decoder) -> ``postprocess`` with the
reference's two timers (inference, NMS; the last batch is not timed), the ``statistics`` triple reduced to rank 0, detections in the
reference's COCO-style ``data_list`` / image-wise dict shapes gathered to rank 0, the return triple ``(ap50_95, ap50, summary)``.

What is different, and why (MI355X): on the GPU the two timed phases of a batch are two HIP-graph replays (the eval forward + reset_net
is ~350 launches whose enqueue time would otherwise bound a 6 ms forward; the post-processing is ``eas_postprocess``, one launch for
the whole batch instead of per-image torchvision NMS).  The graphs are recorded on static input / output buffers per (model, batch
shape) -- the full batch and the short last batch each keep theirs across evaluations -- and dropped when a parameter or buffer of the
model moved.  With a live RCCL process group a capture waits until the group's watchdog thread holds no event
(``yolox.utils.wait_process_group_idle``: a condition read from the flight recorder, not a delay); where that cannot be established
the evaluator launches eagerly.

mAP itself (``COCOeval(gt, dt, 'bbox')`` evaluate -> accumulate -> summarize, :446-461) is computed on the device by ``ops.coco_eval``
(the eas_cocoeval kernels: what the reference's own native module yolox/layers/cocoeval computes, bit for bit) when the model lives on the
GPU: a single process feeds it the device rows of the post-processing directly -- boxes and scores by the torch expressions of
``convert_to_coco_format``, applied on the device -- and with ``distributed=True`` rank 0 uploads the gathered records.  The ground
truths are numbered 0.. in ``gt_dict`` order as getcocoGT numbers them (:365-372).  The return triple is ``(AP, AP50, timings + the twelve
lines of summarize + the per-class AP / AR tables)``.  The Python records, ``return_outputs``, the timers and the statistics are
unchanged.  A model on the CPU, ``EAS_DEVICE_AP=0`` (``ctx.device_ap``) or an input beyond the kernels' limits (the summary names the
reason) take the route of before: pycocotools when importable, else ``None`` AP fields and a summary that says so."""
import itertools
import os
import time
from collections import ChainMap, Counter, defaultdict

import torch

from yolox.utils import gather, get_rank, is_main_process, postprocess, synchronize, time_synchronized, wait_process_group_idle

__all__ = ['EventEvaluator']


def _reset_net(model):
    from spikingjelly.activation_based.functional import reset_net
    reset_net(model)


class _NoGraph(Exception):
    """recording is not safe right now (a live process group whose watchdog cannot be observed): the caller launches eagerly"""


class _GraphedBatch:
    """forward + reset_net as one HIP graph and the device half of the post-processing as a second one, on static buffers"""

    def __init__(self, model, imgs, snn_reset, num_classes, confthre, nmsthre):
        from eas_snn_amd import ops
        self.static_in = imgs.clone()
        self.key = self.signature(model, imgs)
        from eas_snn_amd import _lib
        side = _lib.private_stream()          # the capture stream: never a pooled stream (the process group's stream is one of those)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), ops.no_state_writeback() if snn_reset else _null():
            for _ in range(2):                           # allocator warm-up on the capture stream
                out = model(self.static_in)
                if snn_reset:
                    _reset_net(model)
                ops.postprocess_device(out, num_classes, confthre, nmsthre)
            torch.cuda.synchronize()
            live_group = torch.distributed.is_initialized()
            # ProcessGroupNCCL's watchdog polls the events of collectives it has not retired yet; it must hold none while a capture is
            # open (trainer.py TrainStep.capture).  Wait for that condition; if it cannot be observed, do not record.
            if live_group and not wait_process_group_idle():
                raise _NoGraph()
            self.g_fwd, self.g_post = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            mode = 'thread_local' if live_group else 'global'
            with torch.cuda.graph(self.g_fwd, stream=side, capture_error_mode=mode):
                self.out = model(self.static_in)
                if snn_reset:
                    _reset_net(model)
            if live_group and not wait_process_group_idle():
                raise _NoGraph()
            with torch.cuda.graph(self.g_post, stream=side, capture_error_mode=mode):
                self.rows, self.counts = ops.postprocess_device(self.out, num_classes, confthre, nmsthre)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    @staticmethod
    def signature(model, imgs):
        ptrs = tuple(t.data_ptr() for t in itertools.chain(model.parameters(), model.buffers()))
        return (id(model), tuple(imgs.shape), imgs.device, hash(ptrs))

    def forward(self, imgs):
        self.static_in.copy_(imgs)
        self.g_fwd.replay()
        return self.out

    def post(self):
        self.g_post.replay()
        counts = self.counts.tolist()                    # the one host synchronisation: the result is a ragged list
        return [self.rows[i, :n].clone() if n else None for i, n in enumerate(counts)]


def _per_class_table(per_class, headers, columns=6):
    """name / value pairs laid out ``columns`` cells wide as a pipe table (the layout of per_class_AP_table / per_class_AR_table, :35-80)"""
    from tabulate import tabulate
    cells = [x for item in per_class.items() for x in item]
    width = min(columns, len(cells))
    rows = itertools.zip_longest(*[cells[i::width] for i in range(width)])
    return tabulate(rows, tablefmt='pipe', floatfmt='.3f', headers=headers * (width // len(headers)), numalign='left')


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class EventEvaluator:
    """reference: yolox/evaluators/event_evaluator.py:83-120 (same arguments)."""

    def __init__(self, dataloader, img_size, confthre, nmsthre, num_classes, testdev=False, per_class_AP=True, per_class_AR=True,
                 snn_reset=False):
        self.dataloader = dataloader
        self.img_size = img_size
        self.confthre = confthre
        self.nmsthre = nmsthre
        self.num_classes = num_classes
        self.testdev = testdev
        self.per_class_AP = per_class_AP
        self.per_class_AR = per_class_AR
        # EventExp passes ``use_spike`` here (event_yolox_base.py:533): the option strings 'True' / 'full_spike*' are truthy and so is
        # 'False' in the reference -- resetting a network without neurons is a no-op, so that quirk is harmless and kept
        self.snn_reset = snn_reset
        self.use_graph = os.environ.get('EAS_EVAL_GRAPH', '1') == '1'
        self._graphed = {}                  # signature -> _GraphedBatch (full batch, short last batch)
        self.graphs_recorded = 0
        self.last_statistics = None
        self.last_coco = None               # the ``ops.coco_eval`` result of the last evaluation that computed its AP on the device

    # ------------------------------------------------------------------ the loop
    def evaluate(self, model, distributed=False, half=False, trt_file=None, decoder=None, test_size=None, return_outputs=False):
        """-> (ap50_95, ap50, summary) [, image-wise outputs].  Puts the model into eval mode (like the reference)."""
        if half:
            raise NotImplementedError('the HIP hot path computes in fp32 (reference parity); --fp16 is not provided')
        if trt_file is not None:
            raise NotImplementedError('TensorRT engines do not exist on MI355X; the eval forward is a HIP-graph replay instead')
        model = model.eval()
        ds = getattr(self.dataloader, 'dataset', None)
        assert ds is None or (getattr(ds, 'map_val', True) and not getattr(ds, 'random_aug', False)), \
            'the dataset must be set as the mode of map val. and not random_aug'
        dev = next(model.parameters()).device
        graph_ok = self.use_graph and dev.type == 'cuda' and decoder is None
        if dev.type == 'cuda':
            # nobody writes weights or BatchNorm statistics between the first and the last batch: pack / derive them once (ops.frozen_weights)
            from eas_snn_amd import ops
            with ops.frozen_weights(model):
                return self._evaluate_loop(model, distributed, decoder, return_outputs, dev, graph_ok)
        return self._evaluate_loop(model, distributed, decoder, return_outputs, dev, graph_ok)

    def _run_batches(self, model, decoder, dev, graph_ok, times):
        """the inference loop proper, shared by the evaluators: per batch of the loader forward -> reset_net -> (decoder) -> postprocess,
        as graph replays where possible; yields (outputs, labels, info_imgs, ids) and adds the two timed phases to
        ``times`` = [inference, NMS] seconds"""
        n_batches = len(self.dataloader)
        for cur_iter, (imgs, labels, info_imgs, ids) in enumerate(self.dataloader):
            if len(ids) == 0:                           # an empty batch (the padding of a sharded evaluation): nothing to infer, but the
                yield [], labels, info_imgs, ids        # caller's per-batch work -- a gather with the other ranks -- still takes place
                continue
            with torch.no_grad():                      # (the reference: inference_mode; graph replays write ordinary static buffers)
                imgs = imgs.to(dev, torch.float32)
                # the last batch may be short: not timed, as in the reference (:191-193)
                timed = cur_iter < n_batches - 1
                batch = self._graph_for(model, imgs) if (graph_ok and self.use_graph) else None
                if timed:
                    # the device is idle when the clock starts: the loader's event binning and the copy of the batch above are not "forward"
                    start = time_synchronized()
                if batch is not None:
                    outputs = batch.forward(imgs)
                else:
                    outputs = model(imgs)
                    if self.snn_reset:
                        _reset_net(model)
                    if decoder is not None:
                        outputs = decoder(outputs, dtype=outputs.type())
                if timed:
                    infer_end = time_synchronized()
                    times[0] += infer_end - start
                outputs = batch.post() if batch is not None else postprocess(outputs, self.num_classes, self.confthre, self.nmsthre)
                if timed:
                    nms_end = time_synchronized()
                    times[1] += nms_end - infer_end
            yield outputs, labels, info_imgs, ids

    def _evaluate_loop(self, model, distributed, decoder, return_outputs, dev, graph_ok):
        data_list, output_data, gt_dict = [], {}, {}
        from eas_snn_amd._ctx import ctx
        device_ap = dev.type == 'cuda' and ctx.device_ap
        feed = [] if device_ap and not distributed else None          # single process: the detections stay on the device for the AP
        times = [0.0, 0.0]
        n_samples = max(len(self.dataloader) - 1, 1)
        for outputs, labels, info_imgs, ids in self._run_batches(model, decoder, dev, graph_ok, times):
            if feed is not None and len(ids):                         # (an empty batch, the padding of a sharded evaluation, has no rows)
                self._feed_device_rows(feed, outputs, info_imgs, ids, dev)
            elems, image_wise = self.convert_to_coco_format(outputs, info_imgs, ids, return_outputs=True)
            data_list.extend(elems)
            output_data.update(image_wise)
            for label, height, width, img_id in zip(labels, info_imgs[0], info_imgs[1], ids):
                label = torch.as_tensor(label)
                gt_dict[int(img_id)] = {'bboxes': label[:, :4].tolist(), 'width': int(width), 'height': int(height),
                                        'category_ids': [int(c) for c in label[:, 4]]}
        inference_time, nms_time = times
        statistics = torch.tensor([inference_time, nms_time, n_samples], dtype=torch.float32, device=dev)
        if distributed:
            # ranks finish at different times: meet first, then collect everything on rank 0 (:236-247)
            synchronize()
            data_list = list(itertools.chain(*gather(data_list, dst=0)))
            gt_dict = dict(ChainMap(*gather(gt_dict, dst=0)))
            output_data = dict(ChainMap(*gather(output_data, dst=0)))
            torch.distributed.reduce(statistics, dst=0)
        self.last_statistics = statistics
        eval_results = self.evaluate_prediction(data_list, gt_dict, statistics, device=dev if device_ap else None, feed=feed)
        synchronize()
        if return_outputs:
            return eval_results, output_data
        return eval_results

    def _graph_for(self, model, imgs):
        """the recorded batch for this (model, parameter addresses, input shape); a loader whose last batch is short alternates between two
        signatures in every evaluation -- both stay recorded"""
        key = _GraphedBatch.signature(model, imgs)
        g = self._graphed.get(key)
        if g is None:
            for k in [k for k in self._graphed if k[0] != key[0] or k[3] != key[3]]:
                del self._graphed[k]                    # another model, or this one's tensors moved: free those graphs' pools first
            if len(self._graphed) >= 4:
                self._graphed.pop(next(iter(self._graphed)))
            try:
                g = self._graphed[key] = _GraphedBatch(model, imgs, bool(self.snn_reset), self.num_classes, self.confthre, self.nmsthre)
                self.graphs_recorded += 1
            except _NoGraph:
                self.use_graph = False                  # eager launches from here on (see the module docstring)
                return None
        return g

    # ------------------------------------------------------------------ detections -> COCO-style records (:265-323)
    def convert_to_coco_format(self, outputs, info_imgs, ids, return_outputs=False):
        """rows (x1, y1, x2, y2, obj, cls_conf, cls) per image -> boxes scaled back to the raw sensor size, records
        {image_id, category_id, bbox xywh, score, segmentation}; image-wise {bboxes xyxy, scores, categories}"""
        data_list, image_wise = [], defaultdict(dict)
        for output, img_h, img_w, img_id in zip(outputs, info_imgs[0], info_imgs[1], ids):
            if output is None:
                continue
            output = output.detach().cpu()
            scale = min(self.img_size[0] / float(img_h), self.img_size[1] / float(img_w))
            bboxes = output[:, 0:4] / scale
            cls = output[:, 6]
            scores = output[:, 4] * output[:, 5]
            image_wise[int(img_id)] = {'bboxes': bboxes.tolist(), 'scores': scores.tolist(), 'categories': [int(c) for c in cls]}
            xywh = bboxes.clone()
            xywh[:, 2:4] -= xywh[:, 0:2]
            for box, c, s in zip(xywh.tolist(), cls.tolist(), scores.tolist()):
                data_list.append({'image_id': int(img_id), 'category_id': int(c), 'bbox': box, 'score': s, 'segmentation': []})
        if return_outputs:
            return data_list, image_wise
        return data_list

    def _feed_device_rows(self, feed, outputs, info_imgs, ids, dev):
        """the batch's detections for ``ops.coco_eval`` without leaving the device: (image id int64 [n], class int32 [n], xywh fp32 [n,4],
        score fp32 [n]) by the expressions of ``convert_to_coco_format`` (the division is by a tensor holding the float32 scale: a true
        division like the CPU's, where tensor / python number on the GPU multiplies by the reciprocal)"""
        kept = [k for k, o in enumerate(outputs) if o is not None]
        if not kept:
            return
        rows = torch.cat([outputs[k].detach() for k in kept])
        counts = [outputs[k].shape[0] for k in kept]
        # per-image values go to the device as they are (a few numbers) and are spread over the rows there: a host tensor operation of
        # this many rows would wake the host's thread pool, which then competes with the record loop below for the processors
        per_row = torch.repeat_interleave(torch.arange(len(kept), device=dev), torch.tensor(counts, device=dev), output_size=sum(counts))
        scale = torch.tensor([min(self.img_size[0] / float(info_imgs[0][k]), self.img_size[1] / float(info_imgs[1][k])) for k in kept],
                             dtype=torch.float32, device=dev)[per_row]
        img = torch.as_tensor(ids).to(torch.int64)[kept].to(dev)[per_row]
        bboxes = rows[:, 0:4] / scale[:, None]
        scores = rows[:, 4] * rows[:, 5]
        xywh = bboxes.clone()
        xywh[:, 2:4] -= xywh[:, 0:2]
        feed.append((img, rows[:, 6].to(torch.int32), xywh, scores))

    def _device_ap(self, data_dict, gt_dict, feed, dev, names):
        """-> (ap50_95, ap50, text) from ``ops.coco_eval`` + ``ops.coco_summarize``, or the reason (str) why the kernels decline this input"""
        import numpy as np
        from eas_snn_amd import ops
        image_ids = sorted(gt_dict)
        dense = {i: k for k, i in enumerate(image_ids)}
        gt_img, gt_cls, gt_box = [], [], []
        for i, g in gt_dict.items():                    # annotation ids 0.. in this order (getcocoGT, :365-372)
            for box, c in zip(g['bboxes'], g['category_ids']):
                gt_img.append(dense[i])
                gt_cls.append(c)
                gt_box.append(box)
        per_pair = Counter(zip(gt_img, gt_cls))
        max_gt = max(per_pair.values()) if per_pair else 0
        D = sum(int(f[3].numel()) for f in feed) if feed is not None else len(data_dict)
        G, I, K = len(gt_img), len(image_ids), len(names)
        if not ops.coco_eval_supported(D, G, I, K, max_gt=max_gt):      # asked before anything goes to the device
            return (f'{D} detections, {G} ground truths ({max_gt} in one image and class), {I} images, {K} classes are beyond the limits of '
                    'the eas_cocoeval kernels')
        if feed is not None:
            det_ids = torch.cat([f[0] for f in feed])
            det_cls, det_box, det_score = (torch.cat([f[j] for f in feed]) for j in (1, 2, 3))
        else:                                           # gathered records (rank 0 of a distributed evaluation): uploaded
            det_ids = torch.tensor([d['image_id'] for d in data_dict], dtype=torch.int64, device=dev)
            det_cls = torch.tensor([d['category_id'] for d in data_dict], dtype=torch.int32, device=dev)
            det_box = torch.from_numpy(np.array([d['bbox'] for d in data_dict], np.float32).reshape(-1, 4)).to(dev)
            det_score = torch.from_numpy(np.array([d['score'] for d in data_dict], np.float32)).to(dev)
        # image id -> dense index = its position among the sorted ids (pycocotools: imgIds sorted); an id without ground-truth entry: dropped
        table = torch.tensor(image_ids, dtype=torch.int64, device=dev)
        pos = torch.searchsorted(table, det_ids).clamp_(max=max(I - 1, 0))
        det_img = torch.where(table[pos] == det_ids, pos, torch.full_like(pos, -1)) if I else torch.full_like(det_ids, -1)
        res = ops.coco_eval(det_img, det_cls, det_box, det_score,
                            torch.tensor(gt_img, dtype=torch.int32, device=dev), torch.tensor(gt_cls, dtype=torch.int32, device=dev),
                            torch.tensor(gt_box, dtype=torch.float32, device=dev).reshape(-1, 4), I, K, max_gt=max_gt)
        self.last_coco = dict(res, detections=D, ground_truths=G, images=I)
        stats, lines = ops.coco_summarize(res)
        text = ''.join(line + '\n' for line in lines)
        precision, recall = res['precision'].cpu().numpy(), res['recall'].cpu().numpy()

        def mean100(v):
            v = v[v > -1]
            return float(np.mean(v) * 100) if v.size else float('nan')
        if self.per_class_AP:                           # area range 'all', the last max-dets entry (:58-80)
            text += 'per class AP:\n' + _per_class_table({n: mean100(precision[:, :, k, 0, -1]) for k, n in enumerate(names)}, ['class', 'AP']) + '\n'
        if self.per_class_AR:
            text += 'per class AR:\n' + _per_class_table({n: mean100(recall[:, k, 0, -1]) for k, n in enumerate(names)}, ['class', 'AR']) + '\n'
        return float(stats[0]), float(stats[1]), text

    # ------------------------------------------------------------------ summary (:396-462)
    def _timing_line(self, statistics):
        """'Average forward time: .. ms, Average NMS time: .. ms, Average inference time: .. ms' per sample from the statistics triple"""
        inference_time, nms_time, n_samples = (float(v) for v in statistics.tolist())
        per = 1000.0 / (n_samples * self.dataloader.batch_size)
        a_infer, a_nms = inference_time * per, nms_time * per
        return ', '.join('Average {} time: {:.2f} ms'.format(k, v) for k, v in
                         zip(['forward', 'NMS', 'inference'], [a_infer, a_nms, a_infer + a_nms])) + '\n'

    def evaluate_prediction(self, data_dict, gt_dict, statistics, device=None, feed=None):
        """``device``: where ``ops.coco_eval`` computes the AP (None: the host route); ``feed``: the detections as device arrays
        (``_feed_device_rows``), else ``data_dict`` is uploaded"""
        if not is_main_process():
            return 0, 0, None
        info = self._timing_line(statistics)
        if not data_dict:
            return 0, 0, info
        names = getattr(getattr(self.dataloader, 'dataset', None), 'class_names', None) or [str(i) for i in range(self.num_classes)]
        if device is not None:
            res = self._device_ap(data_dict, gt_dict, feed, device, names)
            if not isinstance(res, str):
                return res[0], res[1], info + res[2]
            info += 'AP on the device declined: ' + res + '\n'
        try:
            from pycocotools.coco import COCO
            from pycocotools.cocoeval import COCOeval
        except ImportError:
            return None, None, info + '{} detections on {} images; pycocotools is not installed: AP not computed\n'.format(
                len(data_dict), len(gt_dict))
        import contextlib
        import io
        gt = COCO()
        gt.dataset = {'images': [{'id': i, 'file_name': str(i), 'width': g['width'], 'height': g['height']} for i, g in gt_dict.items()],
                      'annotations': [], 'categories': [{'id': i, 'name': n, 'supercategory': n} for i, n in enumerate(names)]}
        for i, g in gt_dict.items():
            for box, c in zip(g['bboxes'], g['category_ids']):
                gt.dataset['annotations'].append({'id': len(gt.dataset['annotations']), 'image_id': i, 'category_id': c, 'bbox': box,
                                                  'area': box[2] * box[3], 'iscrowd': 0})
        gt.createIndex()
        ev = COCOeval(gt, gt.loadRes(data_dict), 'bbox')
        ev.evaluate()
        ev.accumulate()
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            ev.summarize()
        return ev.stats[0], ev.stats[1], info + buf.getvalue()
