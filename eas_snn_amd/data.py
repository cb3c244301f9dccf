"""Synthetic event streams and their GPU-side preprocessing (no real datasets in scope).

Stream definition = BASELINE.md section 2 / SURVEY.md 8d: per sample ``n_events`` events over a 200 ms window
on the 240x304 Gen1 sensor, ``t`` sorted uniform, ``x``,``y`` uniform, ``p`` Bernoulli(0.5), numpy default_rng.
Raw events (9 B/event) are what crosses PCIe; binning (K1) and canvas padding run on the GPU.

Further down: the augmentation draws, the N-Caltech101 and 1 Mpx chains, and Gen1 from recordings resident in HBM (``Gen1Store`` and its
loaders: ``.dat`` / ``_bbox.npy`` pairs read once, or seeded synthetic recordings) and N-Caltech101 likewise (``NCaltechStore`` and its
loaders: the split file's recordings and annotation files read once, or seeded synthetic recordings).
"""
import numpy as np
import torch

from . import ops


def synth_event_batch(batch, n_events=200_000, height=240, width=304, t0=1_000_000, span_us=200_000, seed=0):
    """-> dict of numpy arrays (t u32, x u16, y u16, p u8, offsets i64[B+1])."""
    rng = np.random.default_rng(seed)
    n = batch * n_events
    t = np.sort(rng.integers(t0, t0 + span_us, size=(batch, n_events), dtype=np.int64), axis=1).astype(np.uint32).reshape(-1)
    x = rng.integers(0, width, size=n, dtype=np.int64).astype(np.uint16)
    y = rng.integers(0, height, size=n, dtype=np.int64).astype(np.uint16)
    p = (rng.random(n) < 0.5).astype(np.uint8)
    off = np.arange(batch + 1, dtype=np.int64) * n_events
    return dict(t=t, x=x, y=y, p=p, offsets=off)


def events_to_device(ev, device):
    return {k: torch.from_numpy(v).to(device, non_blocking=True) for k, v in ev.items()}


# the values of the reference's ``aggregation`` option (EventExp.aggregation -> slice_args) whose frames the sampler takes: two polarity
# channels, one frame per micro slice
FRAME_AGGREGATIONS = ('micro_sum', 'timesurface')
_OTHER_AGGREGATIONS = ('voxel_grid', 'voxel_cube', 'sum', 'raw_frame')


def check_aggregation(aggregation):
    """``aggregation`` if a device front end has it; ValueError otherwise (nothing trains on another representation without a word)"""
    if aggregation in FRAME_AGGREGATIONS:
        return aggregation
    have = ' and '.join(repr(a) for a in FRAME_AGGREGATIONS)
    why = ''
    if aggregation in _OTHER_AGGREGATIONS:
        why = (f": the reference's {aggregation!r} frames do not have the sampler's two channels per micro slice "
               "(voxel_grid: 1 channel, voxel_cube: 2 * tbins, sum: no micro slices, raw_frame: one frame per timestamp)")
    raise ValueError(f'aggregation {aggregation!r}: the event front ends have {have}{why}')


def unscaled_params(batch, sensor_hw, device):
    """int32 [batch, 5] rows (W, H, 0, 0, 0) made on the device (fills, no copy from the host: graph-capturable): the sensor at scale 1 at
    the top left of a zero canvas, where the count loaders place their frames"""
    par = torch.zeros((batch, 5), dtype=torch.int32, device=device)
    par[:, 0], par[:, 1] = int(sensor_hw[1]), int(sensor_hw[0])
    return par


def _letterboxed(frames, params, canvas_hw, interp='linear'):
    """int32 counts or float64 frames [B, ..., H, W] -> fp32 canvas frames: ``ops.counts_letterbox`` / ``ops.frames_letterbox`` by dtype"""
    op = ops.counts_letterbox if frames.dtype == torch.int32 else ops.frames_letterbox
    return op(frames, params_on(params, frames.device), canvas_hw[0], canvas_hw[1], interp=interp)


def events_to_frames(ev_dev, Tm, sensor_hw, canvas_hw, aggregation='micro_sum', tau=50e3):
    """Device events -> model input [B, Tl=1, Tm, 2, Hc, Wc] fp32 via the HIP histogram (K1).  ``aggregation='timesurface'``: Gen1's
    exponential time surfaces instead (``ops.event_time_surface`` with ``tau`` in us, gen1.py:362-369), placed like the counts: scale 1,
    top left, zero padding (``ops.frames_letterbox`` with ``unscaled_params``).  Any other value raises ValueError."""
    return events_to_frames_augmented(ev_dev, Tm, sensor_hw, canvas_hw, None, aggregation=aggregation, tau=tau)


def synth_targets(batch, canvas_hw, device, n_boxes=2, max_labels=50):
    """[B, 50, 5] rows (cls, cx, cy, w, h), zero padded (yolox/data/.../event_data_augment.py:19-65 contract)."""
    Hc, Wc = canvas_hw
    t = torch.zeros(batch, max_labels, 5)
    boxes = [(0, 0.3, 0.4, 0.25, 0.3), (1, 0.7, 0.6, 0.2, 0.35), (0, 0.5, 0.5, 0.4, 0.4), (1, 0.2, 0.7, 0.15, 0.2)]
    for i in range(min(n_boxes, len(boxes))):
        c, cx, cy, w, h = boxes[i]
        t[:, i] = torch.tensor([c, cx * Wc, cy * Hc, w * Wc, h * Hc])
    return t.to(device)


class SyntheticEventDataset:
    def __init__(self, exp, length=1024, n_events=200_000):
        self.exp, self.length, self.n_events = exp, length, n_events

    def __len__(self):
        return self.length


def exp_aggregation(exp):
    """the experiment's ``aggregation`` field ('micro_sum' without one), checked"""
    return check_aggregation(getattr(exp, 'aggregation', 'micro_sum'))


class SyntheticEventLoader:
    """Iterable of (frames [B,Tl,Tm,2,H,W] fp32 on the GPU, targets [B,50,5]); one 'epoch' = ``iters`` batches.  The frames are those of
    the experiment's ``aggregation`` (``events_to_frames``); a value no front end has raises ValueError, here and when iterating."""

    def __init__(self, exp, batch_size, iters=16, n_events=200_000, sensor_hw=(240, 304)):
        self.exp, self.batch_size, self.iters, self.n_events, self.sensor_hw = exp, batch_size, iters, n_events, sensor_hw
        exp_aggregation(exp)
        self.dataset = SyntheticEventDataset(exp)

    def __len__(self):
        return self.iters

    def close_mosaic(self):
        pass

    def __iter__(self):
        dev = torch.device('cuda', torch.cuda.current_device())
        for i in range(self.iters):
            ev = events_to_device(synth_event_batch(self.batch_size, self.n_events, *self.sensor_hw, seed=i), dev)
            frames = events_to_frames(ev, self.exp.Tm, self.sensor_hw, self.exp.input_size, aggregation=exp_aggregation(self.exp))
            yield frames, synth_targets(self.batch_size, self.exp.input_size, dev)

class SyntheticEvalDataset(SyntheticEventDataset):
    """what the evaluator asks of its dataset (event_evaluator.py:166-169, :348-356): map_val without random augmentation, class / sample names"""
    map_val, random_aug = True, False

    def __init__(self, exp, length=256, n_events=200_000):
        super().__init__(exp, length, n_events)
        self.class_names = [str(i) for i in range(exp.num_classes)]
        self.sample_names = [f'synthetic_{i:06d}' for i in range(length)]
        # opt-in: names that carry a label time, <recording>a<microseconds> (what the Prophesee protocol reads from a Gen1 sample name):
        # sample i is labelled at i * period
        period = getattr(exp, 'eval_label_period_us', None)
        if period:
            self.sample_names = [f'synthetic_{i:06d}a{i * int(period)}' for i in range(length)]


class SyntheticEvalLoader:
    """Iterable of ``(frames [B,Tl,Tm,2,H,W] fp32 on the GPU, labels [B][n,5] rows (x, y, w, h, cls), (heights, widths), ids)`` -- the tuple
    the reference's evaluation loader yields (gen1_collact_func; event_evaluator.py:183).  Sample ``i`` is the seeded stream ``i`` on every
    rank; ``indices`` are this rank's samples (rank, rank + world, ... like DistributedSampler(shuffle=False), event_yolox_base.py:489-494);
    the last batch may be short.  The frames are those of the experiment's ``aggregation``, as in ``SyntheticEventLoader``."""

    def __init__(self, exp, batch_size, indices, n_events=200_000, sensor_hw=(240, 304), dataset=None):
        self.exp, self.batch_size, self.indices, self.n_events, self.sensor_hw = exp, batch_size, list(indices), n_events, sensor_hw
        exp_aggregation(exp)
        self.dataset = dataset if dataset is not None else SyntheticEvalDataset(exp, n_events=n_events)

    def __len__(self):
        return (len(self.indices) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        dev = torch.device('cuda', torch.cuda.current_device())
        H, W = self.sensor_hw
        for b in range(len(self)):
            ids = self.indices[b * self.batch_size:(b + 1) * self.batch_size]
            parts = [synth_event_batch(1, self.n_events, H, W, seed=10_000 + i) for i in ids]
            ev = {k: np.concatenate([p[k] for p in parts]) for k in ('t', 'x', 'y', 'p')}
            ev['offsets'] = np.arange(len(ids) + 1, dtype=np.int64) * self.n_events
            frames = events_to_frames(events_to_device(ev, dev), self.exp.Tm, self.sensor_hw, self.exp.test_size,
                                      aggregation=exp_aggregation(self.exp))
            labels = [torch.tensor([[0.3 * W, 0.4 * H, 0.25 * W, 0.3 * H, float(i % self.exp.num_classes)]]) for i in ids]
            yield frames, labels, (torch.full((len(ids),), H), torch.full((len(ids),), W)), torch.tensor(ids)


# ------------------------------------------------------------------------------------------------ augmentation parameters
def letterbox_params(ih, iw, h, w, letterbox=True, center=False):
    """(nw, nh, dx, dy, flip) of the deterministic branch of GEN1Dataset.get_random_data (gen1.py:438-483)."""
    if letterbox:
        scale = min(w / iw, h / ih)
        nw, nh = int(iw * scale), int(ih * scale)
        dx, dy = ((w - nw) // 2, (h - nh) // 2) if center else (0, 0)
    else:
        nw, nh, dx, dy = w, h, 0, 0
    return nw, nh, dx, dy, 0


def params_on(params, device):
    """per-sample (nw, nh, dx, dy, flip) rows -- a tensor, or anything numpy reads -- as the int32 [B, 5] tensor on ``device`` that the
    kernels take; a tensor that is there already is returned as it is (nothing is read back: graph-capturable)"""
    if not torch.is_tensor(params):
        params = torch.as_tensor(np.asarray(params, dtype=np.int32).reshape(-1, 5))
    return params.to(device)


def jitter_params(ih, iw, h, w, jitter=.3, rng=np.random):
    """(nw, nh, dx, dy, flip) of the random branch of get_random_data (gen1.py:485-504).  Six uniform draws from ``rng`` in the
    reference's order: two for the aspect-ratio distortion (numerator, denominator, each in [1-jitter, 1+jitter)), the scale in
    [0.4, 1), the horizontal and vertical paste offsets, the flip coin."""
    u = lambda lo, hi: lo + (hi - lo) * rng.rand()
    aspect = (iw / ih) * u(1 - jitter, 1 + jitter) / u(1 - jitter, 1 + jitter)
    scale = u(.4, 1)
    if aspect >= 1:                      # wide result: the width is scaled, the height follows the aspect ratio
        nw = int(scale * w)
        nh = int(nw / aspect)
    else:
        nh = int(scale * h)
        nw = int(nh * aspect)
    dx, dy = int(u(0, w - nw)), int(u(0, h - nh))
    return nw, nh, dx, dy, int(u(0, 1) < .5)


def transform_boxes(bboxes, params, ih, iw, h, w, rng=None):
    """Box side of get_random_data (gen1.py:462-473 / :509-520) for given draw results: rows (x1, y1, x2, y2, ...) are
    truncated to int64, optionally shuffled with ``rng``, mapped through the resize / paste / flip (every intermediate result
    truncated to int64 again, as the reference's in-place integer array does), clipped to the canvas, and boxes that are not
    wider and higher than one pixel are dropped.  Returns float32."""
    nw, nh, dx, dy, flip = params
    box = np.array(bboxes, dtype=np.int64)
    if len(box) == 0:
        return box.astype(np.float32)
    if rng is not None:
        rng.shuffle(box)
    xs = (box[:, [0, 2]] * nw / iw + dx).astype(np.int64)        # float64 arithmetic, truncation toward zero
    ys = (box[:, [1, 3]] * nh / ih + dy).astype(np.int64)
    if flip:
        xs = w - xs[:, ::-1]
    box[:, 0], box[:, 2] = np.maximum(xs[:, 0], 0), np.minimum(xs[:, 1], w)
    box[:, 1], box[:, 3] = np.maximum(ys[:, 0], 0), np.minimum(ys[:, 1], h)
    keep = ((box[:, 2] - box[:, 0]) > 1) & ((box[:, 3] - box[:, 1]) > 1)
    return box[keep].astype(np.float32)


# ------------------------------------------------------------------------------------------------ N-Caltech101 (ATIS recordings)
ATIS_OVERFLOW_Y = 240            # a record with this y is no event: it adds ATIS_TIME_INCREMENT to every later time of its recording
ATIS_TIME_INCREMENT = 1 << 13


def encode_atis(t, x, y, p, overflow_before=()):
    """Events -> the byte image of an ATIS recording (N-Caltech101 ``.bin``), numpy uint8 [5 * records].  Record b0..b4: x = b0, y = b1,
    p = b2 >> 7, raw time = (b2 & 127) << 16 | b3 << 8 | b4.  ``overflow_before``: event indices in front of which an overflow record is
    put (``len(t)`` = behind the last event; an index may repeat); the raw times of the events behind it are lowered by 8192 each, so the
    decoded times are ``t`` again.  Every raw time must stay inside 23 bits."""
    t, x, y, p = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (t, x, y, p))
    n = len(t)
    assert len(x) == len(y) == len(p) == n and (y != ATIS_OVERFLOW_Y).all() and ((x >= 0) & (x < 256) & (y >= 0) & (y < 256)).all()
    ov = np.sort(np.asarray(list(overflow_before), dtype=np.int64))
    assert len(ov) == 0 or (ov[0] >= 0 and ov[-1] <= n)
    raw = t - ATIS_TIME_INCREMENT * np.searchsorted(ov, np.arange(n), side='right')
    assert ((raw >= 0) & (raw < (1 << 23))).all(), 'raw ATIS times are 23 bits'
    rec = np.zeros((n + len(ov), 5), dtype=np.uint8)
    pos = np.arange(n) + np.searchsorted(ov, np.arange(n), side='right')          # record index of every event
    rec[pos, 0], rec[pos, 1] = x, y
    rec[pos, 2] = ((p != 0).astype(np.int64) << 7) | (raw >> 16)
    rec[pos, 3], rec[pos, 4] = (raw >> 8) & 255, raw & 255
    is_ov = np.ones(n + len(ov), dtype=bool)
    is_ov[pos] = False
    rec[is_ov, 1] = ATIS_OVERFLOW_Y
    return rec.reshape(-1)


def synth_atis_batch(batch, n_events, height=180, width=240, span_us=300_000, seed=0):
    """-> (bytes uint8 [5 * records], offsets int64 [batch + 1] in records): ``batch`` synthetic ATIS recordings of ``n_events`` events
    each -- ``t`` sorted uniform over ``span_us`` from 0, ``x``, ``y`` uniform on the sensor, ``p`` Bernoulli(0.5) -- with an overflow
    record in front of the first event of every further 65536 us (the 23-bit raw field would not need them at these spans: they are
    there so that the decode is exercised)."""
    rng = np.random.default_rng(seed)
    parts, off = [], [0]
    for _ in range(batch):
        t = np.sort(rng.integers(0, span_us, size=n_events, dtype=np.int64))
        x = rng.integers(0, width, size=n_events, dtype=np.int64)
        y = rng.integers(0, height, size=n_events, dtype=np.int64)
        p = (rng.random(n_events) < 0.5).astype(np.int64)
        marks = np.arange(1, span_us // 65536 + 1) * 65536
        parts.append(encode_atis(t, x, y, p, overflow_before=np.searchsorted(t, marks)))
        off.append(off[-1] + len(parts[-1]) // 5)
    return np.concatenate(parts), np.asarray(off, dtype=np.int64)


ATIS_MEASURES = ('count', 'timesurface')


def atis_to_frames(records_dev, offsets_dev, exp_or_dims, params, interp='cubic', measure=None, tau=500e3, aggregation=None, surface_tau=10e3):
    """Raw ATIS recordings in HBM -> model input [B, Tl, Tm, 2, Hc, Wc] fp32: ``ops.event_histogram_atis`` then ``ops.counts_letterbox``,
    nothing read back in between (graph-capturable).  ``aggregation`` (None: the experiment's ``aggregation`` field, ``'micro_sum'`` without
    one): ``'micro_sum'``, or ``'timesurface'`` = ``ops.event_latest_surface_atis`` with ``surface_tau`` (us) then ``ops.frames_letterbox``,
    the reference's ``aggregation timesurface`` (NCaltech.agrregate, ncaltech.py:255-257); anything else raises ValueError.  With
    ``'timesurface'`` the measure is not consulted, as in the reference, which computes its measure function there and does not use it: the
    rest of this paragraph is about ``'micro_sum'``.  ``measure`` (None: the experiment's ``measure`` field, ``'count'`` without one):
    ``'count'``, or ``'timesurface'`` = ``ops.event_timesurface_atis`` with ``tau`` (us) then ``ops.frames_letterbox``, the reference's
    ``measure timesurface`` (NCaltech.get_measure_func, ncaltech.py:218-225); anything else raises ValueError.  ``exp_or_dims``: an experiment (fields ``Tl``, ``Tm``, ``input_size``, optionally
    ``img_size`` -- the sensor, default (180, 240) -- and ``window`` in ms, as yolox/exp/event_yolox_base.py passes it: ``(window * 1000, 0)``) or a tuple
    ``(Tl, Tm, (H, W), (Hc, Wc))`` with an optional fifth element ``window`` = (lo, hi) in us.  ``params``: per-sample
    (nw, nh, dx, dy, flip) rows, a device int32 tensor or anything numpy reads.  N-Caltech101 resizes every sample, in evaluation too:
    ``letterbox_params(180, 240, 192, 256)`` = (256, 192, 0, 0, 0).  Its random branch (NCaltech.get_random_data, ncaltech.py:330-350)
    is ``jitter_params(..., jitter=.1)``, and the boxes go through ``transform_boxes`` as they are."""
    Tl, Tm, (H, W), canvas_hw, window, kind = _atis_choice(exp_or_dims, measure, aggregation)
    if kind == 'latest':
        frames = ops.event_latest_surface_atis(records_dev, offsets_dev, Tl, Tm, H, W, window=window, tau=surface_tau)
    elif kind == 'timesurface':
        frames = ops.event_timesurface_atis(records_dev, offsets_dev, Tl, Tm, H, W, window=window, tau=tau)
    else:
        frames = ops.event_histogram_atis(records_dev, offsets_dev, Tl, Tm, H, W, window=window)
    return _letterboxed(frames, params, canvas_hw, interp)


def _atis_choice(exp_or_dims, measure=None, aggregation=None):
    """``(Tl, Tm, (H, W), (Hc, Wc), window, kind)`` of ``atis_to_frames``' ``exp_or_dims``, ``kind`` the representation that ``aggregation`` /
    ``measure`` select: ``'latest'`` (aggregation 'timesurface'), ``'timesurface'`` (the measure) or ``'count'``; ValueError for a value no
    front end has, the aggregation first"""
    if isinstance(exp_or_dims, (tuple, list)):
        Tl, Tm, (H, W), (Hc, Wc) = exp_or_dims[:4]
        window = exp_or_dims[4] if len(exp_or_dims) > 4 else None
    else:
        e = exp_or_dims
        Tl, Tm, (H, W), (Hc, Wc) = e.Tl, e.Tm, getattr(e, 'img_size', (180, 240)), e.input_size
        window = (e.window * 1000, 0) if getattr(e, 'window', None) is not None else None
        if measure is None:
            measure = getattr(e, 'measure', None)
        if aggregation is None:
            aggregation = getattr(e, 'aggregation', None)
    if check_aggregation('micro_sum' if aggregation is None else aggregation) == 'timesurface':
        return Tl, Tm, (H, W), (Hc, Wc), window, 'latest'
    measure = 'count' if measure is None else measure
    if measure not in ATIS_MEASURES:
        raise ValueError(f"measure {measure!r}: the N-Caltech101 front end has {' and '.join(repr(m) for m in ATIS_MEASURES)}")
    return Tl, Tm, (H, W), (Hc, Wc), window, measure


def _atis_kind(exp):
    """``kind`` of ``_atis_choice`` for the experiment's ``measure`` / ``aggregation`` alone (ValueError for a value no front end has)"""
    return _atis_choice((1, exp.Tm, (0, 0), (0, 0)), getattr(exp, 'measure', None), getattr(exp, 'aggregation', None))[-1]


# ------------------------------------------------------------------------------------------------ 1 Mpx (RVT stacked histograms)
def rvt_first_index(obj2repr_idx, label_index, num_slice, offset=0):
    """Index of the representation that feeds output slice 0 of a sample: RVTGEN4Dataset.generate_slices' ``start_idx`` (rvt_gen4.py:114-116:
    ``end_idx = objframe_idx_2_repr_idx[time] + 1``, ``start_idx = end_idx - num_slice``) plus the recording's ``offset`` in a store that holds
    several recordings.  May be negative (a young sequence: ``ops.stacked_hist_frames`` fills zero slices in front).  ``obj2repr_idx`` and
    ``label_index`` are numpy arrays / integers on the host or torch tensors on the device; nothing is read back."""
    return obj2repr_idx[label_index] + 1 - num_slice + offset


def gen4_rescale_labels(rows, factor, img_size):
    """The ``rescale`` closure of RVTGEN4Dataset.extract_labels (rvt_gen4.py:370-387) on the rows of one object frame: float32 [L, 7] =
    (t, x, y, w, h, class_id, class_confidence) as the reference makes them; every coordinate times 1 / ``factor`` (down_sample_factor),
    corners clipped to ``img_size`` (h, w) - 1, boxes that lose their area dropped.  Factor 1 or no rows: returned as they are, unclipped,
    like the reference.  Returns a new float32 array."""
    rows = np.array(rows, dtype=np.float32).reshape(-1, 7)
    if len(rows) == 0 or 1.0 / factor == 1:
        return rows
    m = np.float32(1.0 / factor)
    h, w = int(img_size[0]), int(img_size[1])
    x2 = np.clip((rows[:, 1] + rows[:, 3]) * m, 0, w - 1)
    y2 = np.clip((rows[:, 2] + rows[:, 4]) * m, 0, h - 1)
    x1 = np.clip(rows[:, 1] * m, 0, w - 1)
    y1 = np.clip(rows[:, 2] * m, 0, h - 1)
    rows[:, 3], rows[:, 4], rows[:, 1], rows[:, 2] = x2 - x1, y2 - y1, x1, y1
    return rows[(rows[:, 3] > 0) & (rows[:, 4] > 0)]


def gen4_raw_boxes(rows):
    """(x1, y1, x2, y2, class_id) float32 [L, 5] of label rows (t, x, y, w, h, class_id, ...), as RVTGEN4Dataset.__getitem__ builds
    ``raw_bboxes`` (rvt_gen4.py:199-207).  The box side of get_random_data (rvt_gen4.py:510-598, line for line the arithmetic of
    gen1.py:433-521) is ``letterbox_params`` / ``jitter_params(..., jitter=.3)`` and ``transform_boxes`` as they are."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 7)
    return np.stack([rows[:, 1], rows[:, 2], rows[:, 1] + rows[:, 3], rows[:, 2] + rows[:, 4], rows[:, 5]], axis=-1)


def rvt_to_frames(store, first, exp_or_dims, params, lo=None):
    """Representations resident in HBM -> model input [B, 1, Tm, 2, Hc, Wc] fp32 by ``ops.stacked_hist_frames``: one launch, nothing read
    back (graph-capturable when ``first``, ``params`` and ``lo`` are device tensors).  ``store`` u8 [R, 2*nbins, H, W]; ``first`` int64 [B]
    (``rvt_first_index``); ``exp_or_dims``: an experiment (fields ``Tm``, ``input_size``, optionally ``nbins``, default 10) or a tuple
    ``(Tm, (Hc, Wc))`` with an optional third element ``nbins``; ``params``: per-sample (nw, nh, dx, dy, flip) rows, a device int32
    tensor or anything numpy reads, None = the sensor unscaled at the top left (validation at scale 1); ``lo``: first representation of
    each sample's recording (None: 0)."""
    if isinstance(exp_or_dims, (tuple, list)):
        Tm, (Hc, Wc) = exp_or_dims[:2]
        nbins = exp_or_dims[2] if len(exp_or_dims) > 2 else 10
    else:
        Tm, (Hc, Wc), nbins = exp_or_dims.Tm, exp_or_dims.input_size, getattr(exp_or_dims, 'nbins', 10)
    return ops.stacked_hist_frames(store, first, Tm, Hc, Wc, nbins=nbins, lo=lo, params=None if params is None else params_on(params, store.device))


class SyntheticStackedHistLoader:
    """Training loader of the 1 Mpx path on synthetic data: iterable of (frames [B, 1, Tm, 2, Hc, Wc] fp32 on the GPU, targets [B, 50, 5]
    rows (cls, cx, cy, w, h), zero padded -- the layout of ``synth_targets``).  One synthetic recording of ``representations`` stacked
    histograms (u8, Poisson(``rate``) clamped to 255, drawn as ``workloads`` config 4 draws its batch) stays on the device; every
    representation carries one label (objframe_idx_2_repr_idx is the identity) with the boxes of ``raw_boxes``.  An epoch is a permutation
    of the labels; each sample draws its own ``jitter_params(..., jitter=.3)``; frames come from ``rvt_to_frames``, targets from
    ``transform_boxes`` (without the reference's shuffle of a sample's boxes: their order carries nothing).  ``batches(epoch)`` returns
    the draws of an epoch -- a function of (seed, epoch) alone."""

    def __init__(self, exp, batch_size, representations=64, sensor_hw=(360, 640), nbins=10, rate=0.03, seed=0, max_labels=50):
        self.exp, self.batch_size, self.sensor_hw, self.nbins, self.seed, self.max_labels = exp, batch_size, tuple(sensor_hw), nbins, seed, max_labels
        self.representations, self.rate = representations, rate
        self.obj2repr = np.arange(representations, dtype=np.int64)
        self.iters = representations // batch_size
        assert self.iters >= 1, 'fewer labels than one batch'
        self.dataset = SyntheticEventDataset(exp, length=representations)
        self.epoch = 0
        self._store = None

    def __len__(self):
        return self.iters

    def close_mosaic(self):
        pass

    def store(self, device):
        if self._store is None or self._store.device != device:
            g = torch.Generator().manual_seed(1 + self.seed)
            H, W = self.sensor_hw
            hist = torch.poisson(torch.full((self.representations, 2 * self.nbins, H, W), float(self.rate)), generator=g)
            self._store = hist.clamp_(max=255).to(torch.uint8).to(device)
        return self._store

    def raw_boxes(self, label):
        """(x1, y1, x2, y2, class) rows of label ``label`` on the sensor: two boxes that move with the label index"""
        H, W = self.sensor_hw
        s = (int(label) % 8) / 16.0
        nc = max(int(getattr(self.exp, 'num_classes', 2)), 1)
        return np.array([[(0.10 + s) * W, 0.20 * H, (0.35 + s) * W, 0.55 * H, int(label) % nc],
                         [0.50 * W, (0.30 + s / 2) * H, 0.80 * W, (0.60 + s / 2) * H, (int(label) + 1) % nc]], dtype=np.float32)

    def batches(self, epoch):
        """[(label indices int64 [B], params int32 [B, 5])] of an epoch"""
        rs = np.random.RandomState((self.seed * 1_000_003 + epoch) % (1 << 32))
        perm = rs.permutation(self.representations)
        (H, W), (Hc, Wc) = self.sensor_hw, self.exp.input_size
        out = []
        for i in range(self.iters):
            idx = perm[i * self.batch_size:(i + 1) * self.batch_size].astype(np.int64)
            par = np.array([jitter_params(H, W, Hc, Wc, jitter=.3, rng=rs) for _ in idx], dtype=np.int32)
            out.append((idx, par))
        return out

    def targets(self, idx, par):
        """[B, max_labels, 5] float32 (cls, cx, cy, w, h) of the labels ``idx`` under the draws ``par``"""
        (H, W), (Hc, Wc) = self.sensor_hw, self.exp.input_size
        t = np.zeros((len(idx), self.max_labels, 5), dtype=np.float32)
        for b, (label, p) in enumerate(zip(idx, par)):
            box = transform_boxes(self.raw_boxes(label), tuple(int(v) for v in p), H, W, Hc, Wc)[:self.max_labels]
            n = len(box)
            if n:
                t[b, :n, 0] = box[:, 4]
                t[b, :n, 1], t[b, :n, 2] = (box[:, 0] + box[:, 2]) / 2, (box[:, 1] + box[:, 3]) / 2
                t[b, :n, 3], t[b, :n, 4] = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
        return t

    def __iter__(self):
        dev = torch.device('cuda', torch.cuda.current_device())
        store = self.store(dev)
        obj2repr = torch.from_numpy(self.obj2repr).to(dev)
        draws = self.batches(self.epoch)
        self.epoch += 1
        for idx, par in draws:
            first = rvt_first_index(obj2repr, torch.from_numpy(idx).to(dev), self.exp.Tm)
            frames = rvt_to_frames(store, first, (self.exp.Tm, self.exp.input_size, self.nbins), torch.from_numpy(par).to(dev))
            yield frames, torch.from_numpy(self.targets(idx, par)).to(dev)


def events_to_frames_augmented(ev_dev, Tm, sensor_hw, canvas_hw, params, aggregation='micro_sum', tau=50e3):
    """events -> histogram (K1) -> resize / paste / flip on the device -> [B, 1, Tm, 2, Hc, Wc] fp32; ``params``: per-sample
    (nw, nh, dx, dy, flip) rows.  ``aggregation='timesurface'``: ``ops.event_time_surface`` with ``tau`` (us) in place of the histogram,
    then ``ops.frames_letterbox`` (linear, as Gen1 resizes); any value but the two of ``FRAME_AGGREGATIONS`` raises ValueError."""
    H, W = sensor_hw
    ev = ev_dev and (ev_dev['t'], ev_dev['x'], ev_dev['y'], ev_dev['p'], ev_dev['offsets'])
    if check_aggregation(aggregation) == 'timesurface':
        frames = ops.event_time_surface(*ev, Tm, H, W, tau=tau)
    elif params is None:                     # the counts at scale 1, top left: histogram and canvas in one call
        return ops.event_frames(*ev, Tm, H, W, canvas_hw[0], canvas_hw[1]).unsqueeze(1)
    else:
        frames = ops.event_histogram(*ev, Tm, H, W)
    return _letterboxed(frames, unscaled_params(frames.shape[0], sensor_hw, frames.device) if params is None else params, canvas_hw).unsqueeze(1)


def dat_ranges_to_frames(records, ranges, Tm, sensor_hw, canvas_hw, params, aggregation='micro_sum', tau=50e3):
    """The Gen1 chain from record ranges: the .dat image ``records`` in HBM and the ranges int64 [B, 2] of ``ops.event_window_search`` ->
    model input [B, 1, Tm, 2, Hc, Wc] fp32, nothing read back in between (graph-capturable).  ``'micro_sum'``:
    ``ops.event_histogram_dat_ranges`` then ``ops.counts_letterbox``; ``'timesurface'``: ``ops.event_latest_surface_dat_ranges`` with ``tau``
    (us; GEN1Dataset.agrregate, gen1.py:362-369) then ``ops.frames_letterbox``, both with the linear resize; any other value raises
    ValueError.  ``params``: per-sample (nw, nh, dx, dy, flip) rows, a device int32 tensor or anything numpy reads."""
    H, W = sensor_hw
    if check_aggregation(aggregation) == 'timesurface':
        frames = ops.event_latest_surface_dat_ranges(records, ranges, Tm, H, W, tau=tau)
    else:
        frames = ops.event_histogram_dat_ranges(records, ranges, Tm, H, W)
    return _letterboxed(frames, params, canvas_hw).unsqueeze(1)


def packed_ranges_to_frames(table, payload, ranges, Tm, sensor_hw, canvas_hw, params, aggregation='micro_sum', tau=50e3):
    """``dat_ranges_to_frames`` on packed records: ``table`` / ``payload`` of ``ops.records_pack`` and ranges int64 [B, 2] of logical record
    indices -> model input [B, 1, Tm, 2, Hc, Wc] fp32, bit-identical to ``dat_ranges_to_frames`` on the records that were packed; nothing
    read back in between (graph-capturable).  The operators are ``ops.event_histogram_packed_ranges`` /
    ``ops.event_latest_surface_packed_ranges``; everything else is that function's."""
    H, W = sensor_hw
    if check_aggregation(aggregation) == 'timesurface':
        frames = ops.event_latest_surface_packed_ranges(table, payload, ranges, Tm, H, W, tau=tau)
    else:
        frames = ops.event_histogram_packed_ranges(table, payload, ranges, Tm, H, W)
    return _letterboxed(frames, params, canvas_hw).unsqueeze(1)


# ------------------------------------------------------------------------------------------------ stores on N ranks
STORE_SHARD = ('none', 'recordings')        # ``exp.store_shard``: every rank holds every record / a rank holds the records of its own recordings


def shard_recordings(names, weights, world):
    """{name: rank}: the recordings ``names`` (weights ``weights``, anything that orders and adds) dealt out to ``world`` ranks.  Greedy:
    in descending weight (ties: the order given), each to the rank with the least load so far (ties: the lower rank) -- a function of the
    arguments alone, so every rank computes the same assignment without a collective.  When the recording that sets the largest load was
    placed its rank was the least loaded, so ``max load - min load <= largest weight`` and ``max load <= sum / world + largest weight``."""
    names, world = list(names), int(world)
    weights = [int(w) for w in weights]
    if world < 1 or len(weights) != len(names) or len(set(names)) != len(names):
        raise ValueError(f'shard_recordings: {len(names)} names ({len(set(names))} distinct), {len(weights)} weights, world {world}')
    load, out = [0] * world, {}
    for i in sorted(range(len(names)), key=lambda i: -weights[i]):           # (a stable sort: ties stay in the order given)
        r = min(range(world), key=lambda r: load[r])                         # (the first of the least loaded: the lower rank)
        out[names[i]] = r
        load[r] += weights[i]
    return out


def _shard_plan(names, weights, shard, owned):
    """(owned names or None = all, {name: rank} or None) of a store built with ``shard=(rank, world)`` and / or ``owned=``"""
    if shard is None:
        return (None if owned is None else set(owned)), None
    rank, world = int(shard[0]), int(shard[1])
    if not 0 <= rank < world:
        raise ValueError(f'shard = {shard!r}: the rank must lie in [0, world)')
    if owned is not None:
        raise ValueError('give shard= or owned=, not both')
    ranks = shard_recordings(names, weights, world)
    return {n for n, r in ranks.items() if r == rank}, ranks


def _memory_plan(recordings, name, heavy, shard, owned):
    """``_shard_plan`` of recordings in memory: the names are ``name(r)``, the weights ``len(heavy(r))`` (looked at with ``shard=`` only)"""
    if shard is None:
        return _shard_plan((), (), None, owned)
    return _shard_plan([name(r) for r in recordings], [len(heavy(r)) for r in recordings], shard, owned)


def rank_and_world():
    """(rank, world size) as ``yolox.utils`` answers them (from the launcher's parameters while the process group is still deferred)"""
    from yolox import utils
    return int(utils.get_rank()), int(utils.get_world_size())


def exp_store_shard(exp):
    """``(rank, world)`` for the stores of an experiment with ``store_shard = 'recordings'``, None with ``'none'`` (the default); anything
    else raises ValueError"""
    kind = getattr(exp, 'store_shard', 'none')
    if kind not in STORE_SHARD:
        raise ValueError(f'store_shard must be one of {STORE_SHARD}, got {kind!r}')
    return rank_and_world() if kind == 'recordings' else None


def _store_key(exp, split):
    """the key under which ``*_store_for`` keep a store on the experiment: (split, rank, world, store_shard)"""
    return (split,) + rank_and_world() + (getattr(exp, 'store_shard', 'none'),)


def _default_device():
    """the current GPU where there is one, else the host: where ``*_store_for`` build a store when no device is given"""
    return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')


class _Store:
    """What every store of recordings is (``Gen1Store``, ``Gen4Store``, ``NCaltechStore`` and their subclasses): label tables built on the
    host and uploaded once, the samples' names, and what the store knows about the ranks.  A store class states its tables, how it builds
    them (it ends with ``_set_tables`` and ``_set_owners``) and its ``frames``.

    ``host``: numpy copies of the tables, each also a tensor of the same name on ``device``; among them ``boxes`` float32 [L, 5] rows (x1,
    y1, x2, y2, class) on the sensor ``sensor_hw`` and ``group_start`` int64 [G + 1]: sample g has the rows ``group_start[g]`` ..
    ``group_start[g + 1]``.  ``sample_names`` [G]; ``group_rows`` int64 [G] and ``max_group_rows`` (host).  The length is the number of samples.

    The ranks: ``owned_samples`` int64: the ascending global indices of the samples whose records are present (all of them unless the
    store was built with ``owned=`` / ``shard=``); ``owns(indices)``: numpy bool, on the host; ``shard``: the ``(rank, world)`` it was
    built for or None; ``sample_rank`` int32 [G]: the rank that holds every sample's records (None unless built with ``shard=``: with
    ``owned=`` alone the store knows its own recordings only)."""
    shard, sample_rank = None, None
    # what a snapshot (``save`` / ``load_store``) keeps of a store beside ``host``, the names and the owners: the names of its attributes
    # that are ``scalars`` (numbers, None, tuples of numbers), ``lists`` (of strings), ``host`` (numpy arrays) and ``device`` (the tensors on
    # ``self.device`` its ``frames`` reads; one that is None is left out).  A class states its own; ``_loaded`` sets what follows from them.
    _snapshot_fields = dict(scalars=(), lists=(), host=(), device=())

    def _set_tables(self, host):
        """``host`` (a dict of numpy tables with ``group_start`` among them), ``group_rows``, ``max_group_rows``, and every table uploaded
        to ``self.device`` under its name"""
        self.host = host
        self.group_rows = np.diff(host['group_start'])
        self.max_group_rows = int(self.group_rows.max()) if len(self.group_rows) else 0
        for k, v in host.items():
            setattr(self, k, torch.from_numpy(v).to(self.device))

    def _set_owners(self, names, sample_file, owned=None, ranks=None, shard=None):
        """the end of every build: ``names``: the recordings in order; ``sample_file``: the recording of every sample; ``owned``: the names
        whose records are here (None = all); ``ranks``: {name: rank} or None; ``shard``: (rank, world) or None -> ``owned_samples``,
        ``sample_rank``, ``shard``"""
        sample_file = np.asarray(sample_file, dtype=np.int64).reshape(-1)
        self._owner_args, self._owner_ranks = (names, sample_file, owned), ranks
        self._sample_owned = np.array([owned is None or n in owned for n in names], dtype=bool)[sample_file]
        self.owned_samples = np.flatnonzero(self._sample_owned).astype(np.int64)
        self.shard = None if shard is None else (int(shard[0]), int(shard[1]))
        self.sample_rank = None if ranks is None else np.array([ranks[n] for n in names], dtype=np.int32)[sample_file]

    def _adopt(self, shard, ranks):
        """a store built with ``owned=`` from an assignment made outside (from the sizes of files): take ``shard`` = (rank, world) and the
        assignment ``ranks`` = {name: rank} over"""
        if shard is not None:
            self._set_owners(*self._owner_args, ranks, shard)

    @property
    def sharded(self):
        """whether the loaders treat the store as one rank's part of a dataset (a shard of a world of 1 is the whole store)"""
        return (self.shard is not None and self.shard[1] > 1) or len(self.owned_samples) != len(self._sample_owned)

    def owns(self, indices):
        idx = np.asarray(indices, dtype=np.int64)
        ok = (idx >= 0) & (idx < len(self._sample_owned))
        ok[ok] = self._sample_owned[idx[ok]]
        return ok

    def check_owned(self, indices):
        """IndexError for a sample whose records this store does not hold (host; what every loader calls before it uploads indices)"""
        ok = self.owns(indices)
        if not ok.all():
            bad = np.asarray(indices, dtype=np.int64).reshape(-1)[~ok.reshape(-1)]
            raise IndexError(f'samples {bad[:8].tolist()} are not held by this store (shard {self.shard}, {len(self.owned_samples)} of '
                             f'{len(self._sample_owned)} samples owned)')

    def __len__(self):
        return len(self.sample_names)

    def raw_labels(self, index):
        """float32 [n, 5] rows (x, y, w, h, class) of sample ``index`` as the reference's evaluation hands them out (``map_val``,
        ``format='xywh'``: ``xyxy2xywh`` of the raw boxes, gen1.py:191-197, rvt_gen4.py:227-230, ncaltech.py:199-202 -- not truncated, not
        transformed; 1 Mpx: rescaled by extract_labels; N-Caltech101: the sample's one row)"""
        a, b = self.host['group_start'][index], self.host['group_start'][index + 1]
        box = self.host['boxes'][a:b].copy()
        box[:, 2], box[:, 3] = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
        return box

    def targets(self, sample_idx, params, perm, canvas_hw, max_labels=50, return_info=False):
        """[B, max_labels, 5] fp32 rows (cls, cx, cy, w, h), zero padded, of the samples ``sample_idx`` under the draws ``params`` and the
        box permutations ``perm`` (int32 [B, P] or None): ``ops.label_targets`` on the store's box table, one launch, nothing read back"""
        return ops.label_targets(self.boxes, self.group_start, sample_idx, params_on(params, self.device), self.sensor_hw[0], self.sensor_hw[1],
                                 canvas_hw[0], canvas_hw[1], perm=perm, max_labels=max_labels, return_info=return_info)

    def _snapshot_sections(self):
        """[(name, 'host' | 'device', numpy array | tensor)]: the arrays of ``host``, the host arrays the class names, the recording of every
        sample (``_set_owners``' argument), then the device tensors the class names, each at its used size"""
        fields = self._snapshot_fields
        out = [(k, 'host', np.ascontiguousarray(v)) for k, v in self.host.items()]
        out += [(k, 'host', np.ascontiguousarray(getattr(self, k))) for k in fields['host']]
        out.append(('sample_file', 'host', np.ascontiguousarray(self._owner_args[1])))
        return out + [(k, 'device', getattr(self, k)) for k in fields['device'] if getattr(self, k) is not None]

    def save(self, path, key=None, chunk_bytes=None):
        """The store as one snapshot file that ``load_store`` reads back without any of the build's kernels (DESIGN section 3l states the
        format): the magic, a format version, the length of the header, a JSON header -- class, geometry, counters, names, owners, ``key``
        (what ``exp.store_cache`` compares; None outside it) and per section name, dtype, shape, file offset, byte length, place and
        digest -- and the sections as raw little-endian bytes, each on a ``SNAPSHOT_ALIGN`` boundary.  A device section is digested on
        the device (``ops.bytes_digest``), then copied out through one pinned staging buffer of at most ``chunk_bytes`` (None:
        ``SNAPSHOT_CHUNK``).  Written to ``path + '.tmp'`` and moved over ``path`` when complete: a run that is killed leaves no half file
        under the final name.  Returns ``path``."""
        import json
        import os
        import struct
        chunk_bytes = SNAPSHOT_CHUNK if chunk_bytes is None else int(chunk_bytes)
        if chunk_bytes < 1:
            raise ValueError(f'chunk_bytes = {chunk_bytes}')
        fields, sections, entries = self._snapshot_fields, self._snapshot_sections(), []
        for name, where, v in sections:
            flat = torch.from_numpy(v).reshape(-1).view(torch.uint8) if where == 'host' else v.reshape(-1).view(torch.uint8)
            dtype = v.dtype.str if where == 'host' else _snapshot_dtype_name(v.dtype)
            entries.append(dict(name=name, where=where, dtype=dtype, shape=list(v.shape), offset=0, nbytes=flat.numel(),
                                digest=[f'0x{w:016x}' for w in ops.bytes_digest_host(flat)]))
        owner_names, _, owned = self._owner_args
        header = {'class': type(self).__name__, 'format': SNAPSHOT_VERSION,
                  'scalars': {k: getattr(self, k) for k in fields['scalars']}, 'lists': {k: list(getattr(self, k)) for k in fields['lists']},
                  'host_tables': list(self.host), 'host_attrs': list(fields['host']),
                  'names': getattr(self, 'names', None), 'sample_names': list(self.sample_names), 'shard': self.shard,
                  'owners': dict(names=list(owner_names), owned=None if owned is None else sorted(owned), ranks=self._owner_ranks),
                  'key': key, 'sections': entries}
        base = SNAPSHOT_ALIGN
        while True:                                             # the offsets stand in the header whose length moves them
            at = base
            for e in entries:
                e['offset'] = at
                at = _snapshot_aligned(at + e['nbytes'])
            blob = json.dumps(header).encode('utf-8')
            if len(SNAPSHOT_MAGIC) + 12 + len(blob) <= base:
                break
            base += SNAPSHOT_ALIGN
        device_bytes = [e['nbytes'] for e, (_, where, v) in zip(entries, sections) if where == 'device' and v.is_cuda]
        stage = torch.empty(min(chunk_bytes, max(device_bytes)), dtype=torch.uint8, pin_memory=True) if any(device_bytes) else None
        with open(path + '.tmp', 'wb') as f:                    # (a ``.tmp`` an interrupted save left behind is overwritten)
            f.write(SNAPSHOT_MAGIC + struct.pack('<IQ', SNAPSHOT_VERSION, len(blob)) + blob)
            for e, (_, where, v) in zip(entries, sections):
                if e['nbytes'] == 0:
                    continue
                f.seek(e['offset'])
                if where == 'host' or not v.is_cuda:
                    f.write((v if where == 'host' else v.reshape(-1).view(torch.uint8).numpy()).data)
                    continue
                flat = v.reshape(-1).view(torch.uint8)
                for a in range(0, flat.numel(), stage.numel()):
                    n = min(stage.numel(), flat.numel() - a)
                    stage[:n].copy_(flat[a:a + n])              # (blocking: the buffer is read by the write that follows)
                    f.write(stage[:n].numpy().data)
        os.replace(path + '.tmp', path)
        return path

    def _loaded(self):
        """the end of ``load_store``: what follows from the fields a snapshot holds (a class adds its own)"""


SNAPSHOT_MAGIC, SNAPSHOT_VERSION, SNAPSHOT_ALIGN = b'EASSTORE', 1, 4096
SNAPSHOT_CHUNK = 256 << 20                     # bytes of a pinned staging buffer of ``save`` / ``load_store`` unless ``chunk_bytes`` says otherwise
_SNAPSHOT_DTYPES = {'|u1': torch.uint8, '<u2': torch.uint16, '<i4': torch.int32, '<i8': torch.int64, '<f4': torch.float32}


class SnapshotError(ValueError):
    """a snapshot file that is not what was written: a wrong magic or version, a file shorter than its header says, a byte length or a
    digest that does not match.  The message names the file and, where one is at fault, the section."""


def _snapshot_aligned(n):
    return (n + SNAPSHOT_ALIGN - 1) // SNAPSHOT_ALIGN * SNAPSHOT_ALIGN


def _snapshot_dtype_name(dtype):
    for name, t in _SNAPSHOT_DTYPES.items():
        if t == dtype:
            return name
    raise ValueError(f'a snapshot holds no tensors of {dtype}')


def _store_classes(base=None):
    """{name: class} of ``_Store``'s subclasses"""
    out = {}
    for c in (_Store if base is None else base).__subclasses__():
        out[c.__name__] = c
        out.update(_store_classes(c))
    return out


def read_snapshot_header(path):
    """the JSON header of the snapshot ``path`` as a dict, checked as far as it goes without reading a section: magic, version, the
    header's own length, every section's byte length against its dtype and shape and its place against the file's size; ``SnapshotError``
    otherwise"""
    import json
    import os
    import struct
    size = os.path.getsize(path)
    with open(path, 'rb') as f:
        head = f.read(len(SNAPSHOT_MAGIC) + 12)
        if len(head) < len(SNAPSHOT_MAGIC) + 12 or head[:len(SNAPSHOT_MAGIC)] != SNAPSHOT_MAGIC:
            raise SnapshotError(f'{path}: not a store snapshot (the magic is {head[:len(SNAPSHOT_MAGIC)]!r}, not {SNAPSHOT_MAGIC!r})')
        version, length = struct.unpack('<IQ', head[len(SNAPSHOT_MAGIC):])
        if version != SNAPSHOT_VERSION:
            raise SnapshotError(f'{path}: snapshot format version {version}, this code reads version {SNAPSHOT_VERSION}')
        if len(head) + length > size:
            raise SnapshotError(f'{path}: the file holds {size} bytes, its header alone needs {len(head) + length}')
        try:
            header = json.loads(f.read(length).decode('utf-8'))
        except ValueError as e:
            raise SnapshotError(f'{path}: the header is not JSON ({e})') from e
    missing = [k for k in ('class', 'scalars', 'lists', 'host_tables', 'host_attrs', 'names', 'sample_names', 'shard', 'owners', 'key', 'sections')
               if not isinstance(header, dict) or k not in header]
    if missing:
        raise SnapshotError(f'{path}: the header lacks {missing}')
    for e in header['sections']:
        want = int(np.prod(e['shape'], dtype=np.int64)) * np.dtype(e['dtype']).itemsize
        if e['nbytes'] != want:
            raise SnapshotError(f"{path}: section {e['name']!r} states {e['nbytes']} bytes, {e['dtype']} {e['shape']} takes {want}")
        if e['nbytes'] and (e['offset'] % SNAPSHOT_ALIGN or e['offset'] + e['nbytes'] > size):
            raise SnapshotError(f"{path}: section {e['name']!r} lies at {e['offset']} .. {e['offset'] + e['nbytes']}, the file holds {size} bytes")
    return header


def _read_host_section(f, path, e):
    """a section as a numpy array, read in one piece and digested by the numpy path"""
    raw = np.empty(e['nbytes'], dtype=np.uint8)
    f.seek(e['offset'])
    if e['nbytes'] and f.readinto(raw.data) != e['nbytes']:
        raise SnapshotError(f"{path}: section {e['name']!r} ends before its {e['nbytes']} bytes")
    return raw.view(np.dtype(e['dtype'])).reshape(e['shape'])


def _read_device_section(f, path, e, device, chunk_bytes):
    """a section as a tensor on the GPU ``device``, allocated at its exact size and filled from two pinned staging buffers used alternately:
    the file read of chunk k + 1 overlaps the upload of chunk k (``copy_(non_blocking=True)`` on a side stream; the event of a buffer's
    last upload is waited for before the buffer is read into again).  Peak host memory: two chunks."""
    n = e['nbytes']
    flat = torch.empty(n, dtype=torch.uint8, device=device)
    if n:
        chunk = min(int(chunk_bytes), n)
        stage = [torch.empty(chunk, dtype=torch.uint8, pin_memory=True) for _ in range(min(2, (n + chunk - 1) // chunk))]
        done = [None] * len(stage)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))     # (the allocation's earlier life on the current stream is over first)
        f.seek(e['offset'])
        for k, a in enumerate(range(0, n, chunk)):
            b, m = k % len(stage), min(chunk, n - a)
            if done[b] is not None:
                done[b].synchronize()
            if f.readinto(stage[b][:m].numpy().data) != m:
                raise SnapshotError(f"{path}: section {e['name']!r} ends before its {n} bytes")
            with torch.cuda.stream(side):
                flat[a:a + m].copy_(stage[b][:m], non_blocking=True)
                done[b] = torch.cuda.Event()
                done[b].record(side)
        torch.cuda.current_stream(device).wait_stream(side)
        for ev in done:                                         # the staging buffers go back to the allocator: their uploads are over first
            if ev is not None:
                ev.synchronize()
    return flat.view(_SNAPSHOT_DTYPES[e['dtype']]).reshape(e['shape'])


def load_store(path, device, chunk_bytes=None, expect_shard='any'):
    """The store that ``save`` wrote to ``path``, on ``device``, without any of the build's kernels: the class is the header's; the host
    tables are read with numpy and uploaded as ``_set_tables`` uploads them; every device section is allocated at its exact size, filled
    through two pinned staging buffers of at most ``chunk_bytes`` (None: ``SNAPSHOT_CHUNK``; ``_read_device_section``), digested on the
    device and compared with the header.  Peak device memory is the store itself.  ``device='cpu'``: every section is read with numpy and
    digested by the numpy path.  The store equals the built and trimmed one in everything the loaders, the evaluators, ``frames``,
    ``targets``, ``raw_labels``, ``owns`` and ``check_owned`` read; ``capacity_bytes == used_bytes``, ``trim()`` returns the store, there
    is no arena.  It keeps the ``shard`` and the owners it was built with: ``expect_shard`` = a ``(rank, world)`` or None raises
    ``SnapshotError`` when they differ.  ``SnapshotError`` (a ValueError) as well for a file that is not what ``save`` wrote."""
    path, device = str(path), torch.device(device)
    chunk_bytes = SNAPSHOT_CHUNK if chunk_bytes is None else int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError(f'chunk_bytes = {chunk_bytes}')
    header = read_snapshot_header(path)
    cls = _store_classes().get(header['class'])
    if cls is None:
        raise SnapshotError(f"{path}: the snapshot of a {header['class']!r}, which is no store class")
    shard = None if header['shard'] is None else (int(header['shard'][0]), int(header['shard'][1]))
    if expect_shard != 'any' and shard != (None if expect_shard is None else (int(expect_shard[0]), int(expect_shard[1]))):
        raise SnapshotError(f'{path}: the snapshot of shard {shard}, expected {expect_shard}')
    store = cls.__new__(cls)
    store.device = device
    for k, v in header['scalars'].items():
        setattr(store, k, tuple(v) if isinstance(v, list) else v)
    for k, v in header['lists'].items():
        setattr(store, k, list(v))
    if header['names'] is not None:
        store.names = list(header['names'])
    store.sample_names = list(header['sample_names'])
    got = {}
    with open(path, 'rb') as f:
        for e in header['sections']:
            on_gpu = e['where'] == 'device' and device.type == 'cuda'
            if on_gpu:
                got[e['name']] = _read_device_section(f, path, e, device, chunk_bytes)
                words = ops.bytes_digest_host(got[e['name']])
            else:
                got[e['name']] = _read_host_section(f, path, e)
                words = ops.bytes_digest_host(torch.from_numpy(got[e['name']]).reshape(-1).view(torch.uint8))
                if e['where'] == 'device':
                    got[e['name']] = torch.from_numpy(got[e['name']].view(np.uint8)).view(_SNAPSHOT_DTYPES[e['dtype']]).reshape(e['shape'])
            if [f'0x{w:016x}' for w in words] != e['digest']:
                raise SnapshotError(f"{path}: section {e['name']!r} has the digest {[f'0x{w:016x}' for w in words]}, the header states "
                                    f"{e['digest']}: these are not the bytes that were written")
    store._set_tables({k: got[k] for k in header['host_tables']})
    for k in header['host_attrs']:
        setattr(store, k, got[k])
    own = header['owners']
    store._set_owners(own['names'], got['sample_file'], None if own['owned'] is None else set(own['owned']), own['ranks'], shard)
    for k in cls._snapshot_fields['device']:
        setattr(store, k, got.get(k))
    store._loaded()
    return store


class _Arena:
    """The device allocation that a build fills piece by piece, in units of ``unit`` bytes, and the rule of every store that has one: a
    piece that finds no room makes the arena ``full``; from then on the build goes on measuring -- every later piece is still sized,
    nothing more is stored -- and ``close`` raises a ValueError that names the bytes needed.  ``buf`` uint8 [capacity_bytes] (a multiple
    of the unit), ``units``: stored so far = where the next piece goes, ``needed``: measured so far."""

    def __init__(self, capacity_bytes, unit, device):
        self.unit, self.capacity_bytes = unit, capacity_bytes // unit * unit
        self.buf = torch.empty(self.capacity_bytes, dtype=torch.uint8, device=device)
        self.units, self.needed, self.full = 0, 0, False

    def fits(self, units):
        """whether a piece of ``units`` units is stored (at ``self.units``) or only measured"""
        return not self.full and self.units + units <= self.capacity_bytes // self.unit

    def place(self, units):
        """count the next piece, which takes ``units`` units: -> the unit it starts at, None once the arena is full (the caller that
        learns from its pack operator that the piece found no room has set ``full``)"""
        self.needed += units
        self.full = not self.fits(units)
        if self.full:
            return None
        self.units += units
        return self.units - units

    @property
    def used_bytes(self):
        return self.units * self.unit

    def close(self, what):
        """after the build: the view of ``buf`` in use; an arena too small is let go and raises ValueError (``what``: the store's pieces)"""
        if self.full:
            self.buf = None
            raise ValueError(f'the {what} of these recordings need {self.needed * self.unit} bytes, the arena holds {self.capacity_bytes} '
                             '(capacity_bytes)')
        return self.buf[:self.used_bytes]

    def trim(self):
        """reallocate to the used size and let the rest go (old and new exist side by side for the time of the copy) -> the new ``buf``"""
        if self.capacity_bytes != self.used_bytes:
            self.buf, self.capacity_bytes = self.buf[:self.used_bytes].clone(), self.used_bytes
        return self.buf


def _sharded_iters(store, batch_size, rank):
    """steps per epoch of a training loader over a sharded store: the smallest owned count of any rank // the per-rank batch, computed from
    the assignment every rank holds (no collective; all ranks run the same number of steps).  A rank with fewer samples than one batch
    raises ValueError.  A store built with ``owned=`` alone knows only its own count."""
    counts = np.bincount(store.sample_rank, minlength=store.shard[1]) if store.sample_rank is not None else {rank: len(store.owned_samples)}
    for r, n in (counts.items() if isinstance(counts, dict) else enumerate(counts)):
        if n < batch_size:
            raise ValueError(f'rank {r} owns {int(n)} samples, fewer than one batch of {batch_size} (store_shard = recordings)')
    return int(min(counts.values() if isinstance(counts, dict) else counts)) // batch_size


def _shard_state(seed, epoch, rank):
    """the random state of a rank's epoch over a sharded store: MT19937 seeded by the array (seed mod 2^32, epoch, rank) --
    ``init_by_array``, so two different triples never collapse into one integer seed"""
    return np.random.RandomState([int(seed) % (1 << 32), int(epoch), int(rank)])


# ------------------------------------------------------------------------------------------------ Gen1 from recordings resident in HBM
def parse_dat_header(buf):
    """(offset of the first event record, event type, event size) of a Prophesee ``.dat`` file image (bytes or a uint8 array), as the
    reference's reader finds them (psee_loader/io/dat_events_tools.py parse_header): text lines that begin with ``'% '`` form the header; if
    there was at least one, two bytes follow it (event type, event size in bytes); a file without header lines holds type 0 / size 8
    records from its first byte."""
    raw = buf.tobytes() if isinstance(buf, np.ndarray) else bytes(buf)
    pos, lines = 0, 0
    while raw[pos:pos + 2] == b'% ':
        end = raw.find(b'\n', pos)
        lines += 1
        if end < 0:                      # a header line without an end: nothing follows it
            pos = len(raw)
            break
        pos = end + 1
    if lines == 0:
        return pos, 0, 8
    return pos + 2, int(raw[pos]), int(raw[pos + 1])


def encode_dat(t, x, y, p, height=240, width=304):
    """Events -> the byte image of a ``.dat`` recording (uint8 array): the text header, the type / size bytes (0, 8) and one 8-byte record
    per event (uint32 time in us, then x in bits 0..13, y in bits 14..27 and the polarity in bit 28 of a second uint32)."""
    head = ('% Data file containing Event2D events.\n% Version 2\n% Date 2024-1-1 0:0:0\n'
            f'% Height {height}\n% Width {width}\n').encode('latin-1') + bytes([0, 8])
    rec = np.empty((len(t), 2), dtype='<u4')
    rec[:, 0] = t
    rec[:, 1] = (np.asarray(x, np.uint32) & 16383) | ((np.asarray(y, np.uint32) & 16383) << 14) | ((np.asarray(p, np.uint32) & 1) << 28)
    return np.concatenate([np.frombuffer(head, dtype=np.uint8), rec.reshape(-1).view(np.uint8)])


GEN1_BBOX_DTYPE = np.dtype([('t', '<u8'), ('x', '<f4'), ('y', '<f4'), ('w', '<f4'), ('h', '<f4'), ('class_id', 'u1'),
                            ('class_confidence', '<f4'), ('track_id', '<u4')])


def synth_gen1_recordings(n_files, labels_per_file, n_events=50_000, sensor_hw=(240, 304), label_period_us=50_000, num_classes=2, seed=0):
    """``n_files`` seeded recordings ``(name, dat_bytes uint8, bbox_rows)`` as ``Gen1Store`` takes them, so that the store and its loaders
    run without a dataset.  Events: ``t`` sorted uniform over the recording, ``x``, ``y`` uniform on the sensor, ``p`` Bernoulli(0.5).
    Labels: ``labels_per_file`` distinct ascending times, ``label_period_us`` apart, the first one period after the first event; label k
    carries 3, 0 surviving, 1, 2 boxes for k % 4 = 0, 1, 2, 3 -- the label without a survivor holds a box without area and one that lies
    off the sensor, which no resize brings back."""
    H, W = sensor_hw
    out = []
    for f in range(n_files):
        rng = np.random.default_rng([seed, f])
        t0 = 1_000_000 + 10_000 * f
        span = (labels_per_file + 1) * label_period_us
        t = np.sort(rng.integers(t0, t0 + span, size=n_events, dtype=np.int64))
        x, y = rng.integers(0, W, size=n_events), rng.integers(0, H, size=n_events)
        p = (rng.random(n_events) < 0.5).astype(np.int64)
        rows = []
        for k in range(labels_per_file):
            lt = t0 + (k + 1) * label_period_us
            if k % 4 == 1:
                rows += [(lt, 0.4 * W, 0.5 * H, 0.0, 0.0, 0, 1.0, 0), (lt, -0.5 * W, 0.2 * H, 0.2 * W, 0.3 * H, 1 % num_classes, 1.0, 1)]
                continue
            for i in range((3, 0, 1, 2)[k % 4]):
                bw, bh = rng.uniform(0.15, 0.4) * W, rng.uniform(0.15, 0.4) * H
                bx, by = rng.uniform(-0.05, 0.9) * W, rng.uniform(-0.05, 0.9) * H
                rows.append((lt, bx, by, bw, bh, int(rng.integers(0, num_classes)), 1.0, i))
        out.append((f'synthetic_{seed}_{f:03d}', encode_dat(t, x, y, p, H, W), np.array(rows, dtype=GEN1_BBOX_DTYPE)))
    return out


class Gen1Store(_Store):
    """Gen1 recordings and their labels resident on the device: what GEN1Dataset keeps on disk and in host lists (gen1.py:43-85), as tables
    that the kernels index.  ``recordings``: a list of ``(name, dat_bytes, bbox_rows)`` -- the byte image of ``<name>_td.dat`` and the
    structured array of ``<name>_bbox.npy`` (fields ``t`` or ``ts``, ``x``, ``y``, ``w``, ``h``, ``class_id``); names in ``ignore`` are left
    out.  ``Tl``: macro slices per sample (the reference's ``num_slice``); ``window`` = (lo, hi) in us relative to the label time
    (``EventExp.get_slice_args``: ``(window * 1000, 0)``).

    Built once on the host and uploaded once: ``records`` uint8 (the record areas back to back), ``file_offsets`` int64 [F + 1] (record index
    of every recording's first event), ``boxes`` float32 [L, 5] rows (x1, y1, x2, y2, class) (``raw_bboxes``, gen1.py:169-170),
    ``group_start`` int64 [G + 1], ``group_t`` int64 [G] and ``group_file`` int32 [G]: a label group is the rows of one recording that share
    a time, in ascending time (extract_labels, gen1.py:282-298; a descending time raises ValueError).  On the host: ``sample_names``
    ``<name>_r<index>_a<t>`` (get_sample_resp, gen1.py:213-215), ``max_group_rows`` and numpy copies of the tables (``host``).  The flat
    sample index is the group index: recordings in the order given, groups in time order (resolve_index, gen1.py:263-267, with
    ``continuous=True`` as EventExp builds the dataset: no leading groups are dropped).

    On N ranks a store holds the labels of every recording and the records of its own: ``owned`` (a collection of recording names, None
    = all) or ``shard=(rank, world)`` (``shard_recordings`` by ``len(dat_bytes)``; ``recordings`` must be a list then).  A recording that
    is not owned contributes its rows to ``boxes``, ``group_start``, ``group_t``, ``group_file`` and ``sample_names`` -- these, the flat
    sample index, ``raw_labels``, ``targets`` and the length are the same on every rank and the same as the unsharded store's -- and a
    zero-length area to ``records`` / ``file_offsets``; its ``dat_bytes`` may be None and is never touched.  ``owned_samples``, ``owns``,
    ``shard``, ``sample_rank``: see ``_Store``."""
    _snapshot_fields = dict(scalars=('Tl', 'window', 'sensor_hw'), lists=(), host=(), device=('records',))

    def __init__(self, recordings, Tl, window, device, ignore=(), sensor_hw=(240, 304), owned=None, shard=None):
        self._set_geometry(Tl, window, device, sensor_hw)
        areas = []

        def keep(area, times):
            areas.append(area)
            return len(area) // 8
        self._scan(recordings, ignore, keep, owned, shard)
        self.records = torch.from_numpy(np.concatenate(areas) if areas else np.zeros(0, np.uint8)).to(self.device)
        self._set_tables(self.host)

    def _set_geometry(self, Tl, window, device, sensor_hw):
        self.Tl, self.window, self.sensor_hw = int(Tl), (int(window[0]), int(window[1])), (int(sensor_hw[0]), int(sensor_hw[1]))
        self.device = torch.device(device)

    @staticmethod
    def _planned(recordings, ignore, owned, shard):
        """(recordings, owned names or None = all, {name: rank} or None): ``_memory_plan`` by ``len(dat_bytes)``; with ``shard=`` the
        recordings are listed first, without those in ``ignore``"""
        if shard is not None:
            recordings = [r for r in recordings if r[0] not in ignore]
        return (recordings,) + _memory_plan(recordings, lambda r: r[0], lambda r: r[1], shard, owned)

    def _scan(self, recordings, ignore, take, owned=None, shard=None):
        """the label tables (``host``, not uploaded yet, ``names``, ``sample_names``) and the owners of the recordings, taken from the
        iterable one at a time; ``take(record area uint8, label-group times int64)`` is called once per owned recording, in order, and
        returns how many records the store keeps of it (``file_offsets`` is the prefix of those numbers; a recording that is not owned
        adds 0).  Nothing of a recording is held on to here once ``take`` has returned."""
        self.names, self.sample_names = [], []
        tables = dict(file_offsets=[0], boxes=[], group_start=[0], group_t=[], group_file=[])
        recordings, owned, ranks = self._planned(recordings, ignore, owned, shard)
        for name, dat, rows in recordings:
            if name not in ignore:
                self._scan_one(name, dat, rows, tables, take if owned is None or name in owned else None)
            del dat, rows                                       # released before the iterable is asked for the next recording
        self._set_owners(self.names, tables['group_file'], owned, ranks, shard)
        boxes = tables.pop('boxes')
        self.host = dict(file_offsets=np.asarray(tables['file_offsets'], dtype=np.int64),
                         boxes=np.concatenate(boxes).astype(np.float32) if boxes else np.zeros((0, 5), np.float32),
                         group_start=np.asarray(tables['group_start'], dtype=np.int64), group_t=np.asarray(tables['group_t'], dtype=np.int64),
                         group_file=np.asarray(tables['group_file'], dtype=np.int32))

    def _scan_one(self, name, dat, rows, tables, take):
        """``take=None``: a recording that is not owned -- its labels only; ``dat`` is not looked at"""
        if take is not None:
            buf = np.frombuffer(dat, dtype=np.uint8) if isinstance(dat, (bytes, bytearray, memoryview)) else np.asarray(dat, dtype=np.uint8)
            start, _, ev_size = parse_dat_header(buf)
            if ev_size != 8 or (len(buf) - start) % 8 != 0:
                raise ValueError(f'{name}: not a .dat recording of 8-byte event records (event size {ev_size}, {len(buf) - start} bytes)')
        f = len(self.names)
        t = np.asarray(rows['t' if 't' in rows.dtype.names else 'ts']).astype(np.int64)
        if (np.diff(t) < 0).any():
            raise ValueError(f'{name}: the label times are not ascending')
        self.names.append(name)
        first = np.flatnonzero(np.r_[True, np.diff(t) > 0]) if len(t) else np.zeros(0, dtype=np.int64)
        tables['file_offsets'].append(tables['file_offsets'][-1] + (int(take(buf[start:], t[first])) if take is not None else 0))
        tables['boxes'].append(np.stack([rows['x'], rows['y'], rows['x'] + rows['w'], rows['y'] + rows['h'], rows['class_id']], axis=-1)
                               .astype(np.float32).reshape(-1, 5))
        for k, a in enumerate(first):
            self.sample_names.append(f'{name}_r{k}_a{int(t[a])}')
        tables['group_t'] += [int(t[a]) for a in first]
        tables['group_file'] += [f] * len(first)
        base = tables['group_start'][-1]                        # rows of the recordings in front
        tables['group_start'] += [base + int(e) for e in np.r_[first[1:], len(t)]] if len(first) else []

    @classmethod
    def from_directories(cls, paths, Tl, window, device, ignore=(), sensor_hw=(240, 304), shard=None, read_dat=None):
        """the ``<name>_td.dat`` / ``<name>_bbox.npy`` pairs of the directories ``paths``, every directory in sorted order (the reference
        takes them as ``os.listdir`` gives them), read with ``numpy.fromfile`` / ``numpy.load``.  ``shard=(rank, world)``: every recording is
        listed and weighed by the size of its ``_td.dat`` (``os.path.getsize``: nothing of a recording is read for the assignment), every
        ``_bbox.npy`` is read, and of the ``_td.dat`` files only those ``shard_recordings`` gives to ``rank``.  ``read_dat(path)``: the reader
        of a ``_td.dat`` (default ``numpy.fromfile(path, dtype=numpy.uint8)``)."""
        pairs, owned, ranks = cls._listed(paths, ignore, shard)
        store = cls(list(cls._read(pairs, owned, read_dat)), Tl, window, device, sensor_hw=sensor_hw, owned=owned)
        store._adopt(shard, ranks)
        return store

    @staticmethod
    def _listed(paths, ignore, shard):
        """([(name, path of _td.dat, path of _bbox.npy)] in the order of ``from_directories``, owned names or None, {name: rank} or None)"""
        import os
        pairs = [(fn[:-len('_bbox.npy')], os.path.join(path, fn[:-len('_bbox.npy')] + '_td.dat'), os.path.join(path, fn))
                 for path in ([paths] if isinstance(paths, str) else paths) for fn in sorted(os.listdir(path))
                 if fn.endswith('_bbox.npy') and fn[:-len('_bbox.npy')] not in ignore]
        owned, ranks = _shard_plan([p[0] for p in pairs], [os.path.getsize(p[1]) for p in pairs] if shard is not None else (), shard, None)
        return pairs, owned, ranks

    @classmethod
    def _source_files(cls, paths, ignore, shard):
        """the files ``from_directories`` with these arguments would open, from the listing alone: every ``_bbox.npy``, the owned ``_td.dat``"""
        pairs, owned, _ = cls._listed(paths, ignore, shard)
        return [box for _, _, box in pairs] + [dat for name, dat, _ in pairs if owned is None or name in owned]

    @staticmethod
    def _read(pairs, owned, read_dat=None):
        """the recordings ``(name, dat_bytes or None where not owned, bbox_rows)`` of the listed ``pairs``, read one at a time as they are
        asked for"""
        read_dat = read_dat if read_dat is not None else (lambda p: np.fromfile(p, dtype=np.uint8))
        for name, dat, box in pairs:
            yield name, read_dat(dat) if owned is None or name in owned else None, np.load(box)

    def _window_times(self, t):
        """int64 [G * Tl]: the ends of the ``Tl`` windows that end at the label times ``t`` (int64 [G] on the device), a window apart"""
        shift = torch.arange(-self.Tl + 1, 1, dtype=torch.int64, device=self.device) * (self.window[1] - self.window[0])
        return (t[:, None] + shift[None, :]).reshape(-1)

    def frames(self, sample_idx, params, exp, canvas_hw=None):
        """model input [B, Tl, Tm, 2, Hc, Wc] fp32 of the samples ``sample_idx`` (int64 [B] on the device): label time and recording gathered
        on the device, ``ops.event_window_search`` for the ``Tl`` windows that end at the label (generate_slices with ``continuous``,
        gen1.py:117-125), then ``dat_ranges_to_frames`` with the experiment's ``aggregation``; ``params``: (nw, nh, dx, dy, flip) per
        sample; ``canvas_hw``: ``exp.input_size`` unless given.  Nothing is read back (graph-capturable).  Precondition: the store
        holds the records of every sample asked for (``owns``; the loaders check their indices on the host before they upload them) -- a
        sample that is not owned has no records here and comes out as empty frames, silently."""
        B, Tl = sample_idx.numel(), self.Tl
        t = self._window_times(self.group_t[sample_idx])
        f = self.group_file[sample_idx][:, None].expand(B, Tl).reshape(-1)
        ranges = ops.event_window_search(self.records, t, self.window, Tl, self.file_offsets, f)
        par = params_on(params, self.device)[:, None, :].expand(B, Tl, 5).reshape(-1, 5)
        Hc, Wc = canvas_hw if canvas_hw is not None else exp.input_size
        out = dat_ranges_to_frames(self.records, ranges, exp.Tm, self.sensor_hw, (Hc, Wc), par, aggregation=exp_aggregation(exp))
        return out.reshape(B, Tl, exp.Tm, 2, Hc, Wc)


class Gen1WindowStore(Gen1Store):
    """A ``Gen1Store`` that keeps of every recording only the records its samples read: the ``Tl`` windows of ``|window|`` us that end at
    a label (with the reference's 200 ms window and labels a few times per second at most, a fraction of a recording).  Tables,
    ``sample_names``, ``raw_labels``, ``targets`` and the length are the parent's; ``frames`` is bit-identical to the parent's.

    Which records a window holds depends on the whole recording (the reader's bisection probes, its resets and its steps back,
    ``ops.event_window_search``), so the search runs on the full recording, once, at build time.  ``recordings`` is any iterable of ``(name,
    dat_bytes, bbox_rows)`` and is consumed one recording at a time: upload, ``ops.event_window_search`` for all its label groups x ``Tl``
    windows (the arguments ``Gen1Store.frames`` uses), ``ops.record_ranges_union``, ``ops.records_gather`` into an arena, and the upload is
    freed -- the device holds the arena and one recording, the host whatever the iterable holds.  Results: ``records`` uint8 (the kept
    areas back to back), ``file_offsets`` int64 [F + 1] of the kept areas (a recording without labels keeps nothing), ``sample_ranges`` int64
    [G, Tl, 2] (record indices into ``records`` of every sample's windows; an empty window is an empty range) and the host ints
    ``total_records``, ``kept_records``, ``capacity_bytes``, ``used_bytes``.

    ``capacity_bytes``: the arena's size; None = 0.8 x the free device memory at the start, or ``source_bytes`` (what the caller knows the
    record areas to add up to at most; measured here when ``recordings`` is a list or tuple) if that is less.  When the arena is too small
    the remaining recordings are still scanned, nothing more is stored, and a ValueError names the bytes needed.  ``trim()`` gives back
    what is not used.

    ``owned`` / ``shard`` as in ``Gen1Store``: a recording that is not owned is neither uploaded nor searched, keeps nothing, and its
    samples carry empty ranges in ``sample_ranges`` (which stays [G, Tl, 2] over the global sample index); ``total_records`` and
    ``kept_records`` count the owned recordings, so the ranks' ``kept_records`` add up to the unsharded store's.  ``shard=`` weighs a
    recording by ``len(dat_bytes)``, which is only a proxy for what its windows keep: the balance bound of ``shard_recordings`` holds
    for the bytes read at build time, not for the bytes held."""
    _snapshot_fields = dict(Gen1Store._snapshot_fields, scalars=Gen1Store._snapshot_fields['scalars'] + ('total_records', 'kept_records', 'used_bytes'),
                            device=('records', 'sample_ranges'))

    def __init__(self, recordings, Tl, window, device, ignore=(), sensor_hw=(240, 304), capacity_bytes=None, source_bytes=None, owned=None,
                 shard=None):
        self._set_geometry(Tl, window, device, sensor_hw)
        if capacity_bytes is None:
            if source_bytes is None:
                recordings, mine, _ = self._planned(recordings, ignore, owned, shard)
                if isinstance(recordings, (list, tuple)):
                    source_bytes = sum(len(dat) for name, dat, _ in recordings if mine is None or name in mine)
            capacity_bytes = self._default_capacity(source_bytes)
        self._open_arena(int(capacity_bytes))
        self.capacity_bytes = self._arena.capacity_bytes
        self.total_records, self.kept_records, self._ranges = 0, 0, []
        self._scan(recordings, ignore, self._compact, owned, shard)
        self._close_arena()
        self.used_bytes = self._arena.used_bytes
        ranges, self._ranges = self._ranges, None
        if self.sharded:                                                # the rows of the owned samples, in their order; the others stay empty
            self.sample_ranges = torch.zeros((len(self.sample_names), self.Tl, 2), dtype=torch.int64, device=self.device)
            if ranges:
                self.sample_ranges[torch.from_numpy(self.owned_samples).to(self.device)] = torch.cat(ranges)
        else:
            self.sample_ranges = torch.cat(ranges) if ranges else torch.zeros((0, self.Tl, 2), dtype=torch.int64, device=self.device)
        self._set_tables(self.host)

    def _open_arena(self, capacity_bytes):
        self._arena = _Arena(capacity_bytes, 8, self.device)            # a unit is a record

    def _close_arena(self):
        """after the scan: the view of the arena that holds the records, or the ValueError of an arena too small"""
        self.records = self._arena.close('windows')

    def _default_capacity(self, source_bytes):
        free = int(0.8 * torch.cuda.mem_get_info(self.device)[0]) if self.device.type == 'cuda' else None
        if free is None and source_bytes is None:
            raise ValueError('capacity_bytes (or source_bytes) must be given where the free device memory cannot be asked for')
        return min(v for v in (free, source_bytes) if v is not None)

    def _window_union(self, area, times):
        """(the recording on the device, segments, seg_dst, mapped): upload, ``ops.event_window_search`` for every label group x ``Tl``
        windows, ``ops.record_ranges_union``.  ``area``: the record area (uint8, host), not empty; ``times``: its label-group times."""
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', UserWarning)                # a read-only host array is only read
            rec = torch.from_numpy(area).to(self.device)
        ranges = ops.event_window_search(rec, self._window_times(torch.from_numpy(times).to(self.device)), self.window, self.Tl)
        return (rec,) + ops.record_ranges_union(ranges)

    def _window_ranges(self, area, times):
        """(ranges int64 [G * Tl, 2] into the arena from record 0 of this recording's kept area, records kept): the device steps of one
        recording, the gather into the arena -- where it still has room -- among them"""
        rec, segments, seg_dst, mapped = self._window_union(area, times)
        kept = int(seg_dst[-1])
        if self._arena.fits(kept):
            ops.records_gather(rec, segments, seg_dst, self._arena.buf, self._arena.units)
        return mapped, kept

    def _placed(self, kept):
        """(index of the first, number) of the records that ``records`` / ``file_offsets`` / ``sample_ranges`` count for a recording of
        ``kept`` kept records, None once the arena is full"""
        at = self._arena.place(kept)
        return None if at is None else (at, kept)

    def _compact(self, area, times):
        """``_scan``'s ``take``: one recording measured and, while the arena has room, stored"""
        self.total_records += len(area) // 8
        if len(times) == 0:
            return 0
        if len(area) == 0:                                              # no events: every window is empty
            mapped, kept = torch.zeros((len(times) * self.Tl, 2), dtype=torch.int64, device=self.device), 0
        else:
            mapped, kept = self._window_ranges(area, np.ascontiguousarray(times, dtype=np.int64))
        placed = self._placed(kept)
        if placed is None:                                              # too small: go on measuring, store nothing more
            return 0
        self._ranges.append((mapped + placed[0]).reshape(len(times), self.Tl, 2))
        self.kept_records += kept
        return placed[1]

    @classmethod
    def from_directories(cls, paths, Tl, window, device, ignore=(), sensor_hw=(240, 304), capacity_bytes=None, shard=None, read_dat=None):
        """the ``<name>_td.dat`` / ``<name>_bbox.npy`` pairs of the directories ``paths`` as ``Gen1Store.from_directories`` lists them, read
        one at a time while the store is built: the host holds one recording.  ``shard`` and ``read_dat`` as there: only the owned
        ``_td.dat`` files are read (their size is the weight -- a proxy for what the windows keep, see the class)."""
        import os
        pairs, owned, ranks = cls._listed(paths, ignore, shard)
        size = sum(os.path.getsize(dat) for name, dat, _ in pairs if owned is None or name in owned)
        store = cls(cls._read(pairs, owned, read_dat), Tl, window, device, sensor_hw=sensor_hw, capacity_bytes=capacity_bytes, source_bytes=size,
                    owned=owned)
        store._adopt(shard, ranks)
        return store

    def _loaded(self):
        self.capacity_bytes = self.used_bytes                           # every section was allocated at its size: there is no arena

    def trim(self):
        """give back what the arena does not use: its bytes in use are reallocated at their size (``_Arena.trim``); a store that
        ``load_store`` made has nothing to give back"""
        if getattr(self, '_arena', None) is None:
            return self
        self.records, self.capacity_bytes = self._arena.trim(), self._arena.used_bytes
        return self

    def frames(self, sample_idx, params, exp, canvas_hw=None):
        """model input [B, Tl, Tm, 2, Hc, Wc] fp32 of the samples ``sample_idx`` (int64 [B] on the device), as ``Gen1Store.frames`` gives
        it: the windows come from ``sample_ranges`` -- no search, nothing read back (graph-capturable).  The store was built for one
        ``(Tl, window)``: an experiment that carries another raises ValueError.  The precondition on ``sample_idx`` is the parent's."""
        asked = (int(getattr(exp, 'Tl', self.Tl)), (int(exp.window * 1000), 0) if hasattr(exp, 'window') else self.window)
        if asked != (self.Tl, self.window):
            raise ValueError(f'the store was built for Tl = {self.Tl} and the window {self.window} us, the experiment asks for Tl = {asked[0]} '
                             f'and {asked[1]}')
        B, Tl = sample_idx.numel(), self.Tl
        par = params_on(params, self.device)[:, None, :].expand(B, Tl, 5).reshape(-1, 5)
        Hc, Wc = canvas_hw if canvas_hw is not None else exp.input_size
        out = self._frames_from(self.sample_ranges[sample_idx].reshape(-1, 2), exp.Tm, (Hc, Wc), par, exp_aggregation(exp))
        return out.reshape(B, Tl, exp.Tm, 2, Hc, Wc)

    def _frames_from(self, ranges, Tm, canvas_hw, params, aggregation):
        return dat_ranges_to_frames(self.records, ranges, Tm, self.sensor_hw, canvas_hw, params, aggregation=aggregation)


class Gen1PackedWindowStore(Gen1WindowStore):
    """``Gen1WindowStore`` with the kept records in packed form (include/eas_hip.h states the format): blocks of 64 records, a narrow
    block -- coordinates inside the sensor, times within ``2^DB - 1`` us of the block's minimum; DB = 14 on Gen1 -- as 64 words of 4 bytes,
    any other block as its 64 records.  ``table`` int32 [NB, 2] (the bit patterns of base time and unit | wide << 31), ``payload`` uint8
    [used_bytes]; ``records`` stays None.  The frames are bit-identical to the parent's (``packed_ranges_to_frames``: the parent's range
    kernels with the packed records as their source); tables, names, ``raw_labels``, ``targets``, ``owned`` / ``shard`` and
    ``from_directories`` are the parent's.

    The build, per recording, is the parent's up to the gather, which goes into a scratch of that recording's kept records;
    ``ops.records_pack`` packs the scratch behind the arena's current unit.  Every recording starts on a fresh block: ``sample_ranges`` and
    ``file_offsets`` are LOGICAL record indices (block * 64 + lane), and the padding behind a recording's last record lies in no range.
    The device holds the arena, the table, one recording and that recording's kept records.  ``capacity_bytes``: the arena's size (None:
    the parent's rule -- the source's size bounds what any packing needs up to 512 bytes per recording); the table is allocated beside it,
    8 bytes per 256 of the arena.  An arena that is too small raises ValueError naming the bytes needed, after everything was measured.
    ``used_bytes``: the payload in use; ``nbytes()``: payload + table; ``narrow_blocks`` / ``wide_blocks``; ``kept_records`` and
    ``total_records`` count records as the parent does; ``unpacked(a, e)``: logical records [a, e) as 8-byte records; ``trim()`` gives the
    rest of the arena and of the table back.  A sensor that leaves fewer than 8 bits for the time raises ValueError."""
    _snapshot_fields = dict(Gen1WindowStore._snapshot_fields, scalars=Gen1WindowStore._snapshot_fields['scalars'] + ('narrow_blocks', 'wide_blocks'),
                            device=('table', 'payload', 'sample_ranges'))

    def _loaded(self):
        super()._loaded()
        self.records, self._table, self._blocks = None, self.table, self.table.shape[0]

    def _open_arena(self, capacity_bytes):
        ops.records_widths(*self.sensor_hw)
        self.records = None
        self._arena = _Arena(capacity_bytes, ops.RECORDS_UNIT, self.device)
        self._table = torch.empty((self._arena.capacity_bytes // ops.RECORDS_UNIT, 2), dtype=torch.int32, device=self.device)  # a block takes a unit at least
        self._blocks = 0

    def _window_ranges(self, area, times):
        """(ranges int64 [G * Tl, 2] of logical records from this recording's first block, records kept); the kept records are gathered
        into a scratch and packed behind the arena's current unit, or only measured once the arena is full"""
        rec, segments, seg_dst, mapped = self._window_union(area, times)
        kept = int(seg_dst[-1])
        if kept:
            scratch = torch.empty(8 * kept, dtype=torch.uint8, device=self.device)
            ops.records_gather(rec, segments, seg_dst, scratch)
            arena, nb = self._arena, self._blocks_of(kept)
            arena.full = arena.full or self._blocks + nb > self._table.shape[0]      # (more blocks than the arena has units: it cannot take them either)
            table = torch.empty((nb, 2), dtype=torch.int32, device=self.device) if arena.full else self._table[self._blocks:self._blocks + nb]
            try:
                took = ops.records_pack(scratch, table, arena.buf, arena.units, *self.sensor_hw, dry_run=arena.full)
            except ops.PackedArenaFull as e:                                # too small: go on measuring, store nothing more
                took, arena.full = e.units, True
            arena.place(took)
        return mapped, kept

    @staticmethod
    def _blocks_of(kept):
        return (kept + ops.RECORDS_BLOCK - 1) // ops.RECORDS_BLOCK

    def _placed(self, kept):
        """the parent's, in logical records: every recording starts on a fresh block (``_window_ranges`` has placed its units already)"""
        if self._arena.full:
            return None
        first, nb = self._blocks * ops.RECORDS_BLOCK, self._blocks_of(kept)
        self._blocks += nb
        return first, nb * ops.RECORDS_BLOCK

    def _close_arena(self):
        self.payload = self._arena.close('packed records')
        self.table = self._table[:self._blocks]
        self.wide_blocks = self._arena.units - self._blocks             # a narrow block takes one unit, a wide block two
        self.narrow_blocks = self._blocks - self.wide_blocks

    def nbytes(self):
        """bytes of the payload in use and of the table"""
        return self.used_bytes + self.table.numel() * 4

    def trim(self):
        """the parent's, for ``payload``; the table is reallocated at its used size with it"""
        if getattr(self, '_arena', None) is None:
            return self
        if self.capacity_bytes != self.used_bytes:
            self.table = self._table = self.table.clone()
        self.payload, self.capacity_bytes = self._arena.trim(), self._arena.used_bytes
        return self

    def unpacked(self, a, e):
        """uint8 [8 * (e - a)]: the logical records ``a`` .. ``e`` as the parent holds them (8-byte records)"""
        return ops.records_unpack(self.table, self.payload, a, e, *self.sensor_hw)

    def _frames_from(self, ranges, Tm, canvas_hw, params, aggregation):
        return packed_ranges_to_frames(self.table, self.payload, ranges, Tm, self.sensor_hw, canvas_hw, params, aggregation=aggregation)


STORE_RECORDS = ('all', 'windows')          # ``exp.store_records``: every record of the recordings (Gen1Store) / those the samples read
STORE_EVENTS = ('dat', 'packed')            # ``exp.store_events``: the kept records as 8-byte .dat records / packed (Gen1PackedWindowStore)


def _data_dirs(exp, split):
    """[``exp.data_dir``/train, /val] (``split='test'``: [/test]) when every one of them is a directory, else None"""
    import os
    root = str(getattr(exp, 'data_dir', '') or '')
    dirs = [os.path.join(root, d) for d in (('test',) if split == 'test' else ('train', 'val'))]
    return dirs if root and all(os.path.isdir(d) for d in dirs) else None


def _store_for(exp, attr, split, device, find, from_data, synthetic, more=(), snapshot=None):
    """What the three ``*_store_for`` share: the stores kept on the experiment in the dict ``attr``, one per ``_store_key(exp, split)`` +
    ``more``; a store that is not there yet is built on ``device`` (None: ``_default_device()``) with the shard of the
    experiment (``exp_store_shard``) -- ``from_data(found, device, shard)`` if ``find()`` finds the dataset, else ``synthetic(device, shard)``.
    With ``exp.store_cache`` (a directory; None, the default: no cache) a store of a dataset that was found comes from its snapshot there
    where that is current, and leaves one where it is not (``_store_from_cache``; ``snapshot(found, shard)`` -> (``train_input``, the store
    class, the constructor arguments that shape the store, the directory the source paths are relative to, the source files)).  Synthetic
    stores are never cached."""
    cache = exp.__dict__.setdefault(attr, {})
    shard = exp_store_shard(exp)
    key = _store_key(exp, split) + more
    if key not in cache:
        device = _default_device() if device is None else device
        found = find()
        if not found:
            cache[key] = synthetic(device, shard)
        elif snapshot is None or not getattr(exp, 'store_cache', None):
            cache[key] = from_data(found, device, shard)
        else:
            cache[key] = _store_from_cache(str(exp.store_cache), split, device, shard, *snapshot(found, shard),
                                           lambda: from_data(found, device, shard))
    return cache[key]


def snapshot_key(cls, args, shard, root, files):
    """What a snapshot of ``exp.store_cache`` is current by, computed without reading a source file: the format version, the store class,
    the constructor arguments that shape the store, the shard, and (path relative to ``root``, size, ``mtime_ns``) of every source file;
    in the form JSON gives it back (lists, no tuples), so that it compares equal to the ``key`` of a header"""
    import json
    import os
    sources = []
    for p in files:
        st = os.stat(p)
        sources.append([os.path.relpath(p, root), st.st_size, st.st_mtime_ns])
    return json.loads(json.dumps(dict(format=SNAPSHOT_VERSION, cls=cls.__name__, args=args, shard=shard, sources=sources)))


def snapshot_name(train_input, split, key, shard):
    """``<train_input>_<split>_<first 16 hex digits of the sha256 of the key>[_r<rank>of<world>].eas``; the rank only for a sharded store"""
    import hashlib
    import json
    digest = hashlib.sha256(json.dumps(key, sort_keys=True).encode('utf-8')).hexdigest()[:16]
    return f'{train_input}_{split}_{digest}' + ('' if shard is None else f'_r{int(shard[0])}of{int(shard[1])}') + '.eas'


def _store_from_cache(directory, split, device, shard, train_input, cls, args, root, files, build):
    """The store from its snapshot in ``directory`` if a file of the key's name is there, its header carries the key and ``load_store``
    accepts it; otherwise ``build()`` and, from the rank that writes, ``save`` under that name.  A ``SnapshotError`` is warned about once,
    then the store is built and the file overwritten.  Every rank of a sharded world (``shard``) writes its own file; in replica mode only
    rank 0 writes, and another rank that finds no file builds without waiting -- the process group may not exist yet, so no collective."""
    import os
    import warnings
    key = snapshot_key(cls, args, shard, root, files)
    path = os.path.join(directory, snapshot_name(train_input, split, key, shard))
    if os.path.exists(path):
        try:
            if read_snapshot_header(path).get('key') == key:
                return load_store(path, device, expect_shard=shard)
        except SnapshotError as e:
            warnings.warn(f'{e}; the store is built from the dataset and the snapshot written again')
    store = build()
    if shard is not None or rank_and_world()[0] == 0:
        os.makedirs(directory, exist_ok=True)
        store.save(path, key=key)
    return store


def gen1_store_for(exp, split='train', device=None):
    """The store of an experiment with ``train_input = 'dat_store'``: ``Gen1Store.from_directories`` over ``exp.data_dir``/train + /val
    (``split='test'``: /test) when that directory exists, seeded synthetic recordings otherwise (``exp.store_recordings`` = (files, labels
    per file, events per file), default (4, 16, 50000); the sensor is Gen1's, or the canvas where that is smaller).  ``exp.store_records``
    (default ``'all'``) = ``'windows'``: a ``Gen1WindowStore``, trimmed; any other value raises ValueError.  ``exp.store_shard`` =
    ``'recordings'``: the store of this rank (``shard=`` of ``from_directories`` / of the constructor for the synthetic recordings).
    ``exp.store_events`` (default ``'dat'``) = ``'packed'`` with ``store_records = 'windows'``: a ``Gen1PackedWindowStore``, trimmed;
    ``'packed'`` with ``store_records = 'all'``, or any other value, raises ValueError before any device work.  Kept on the experiment: one
    store per (split, rank, world, store_shard), the three kinds of store apart."""
    kind, events = getattr(exp, 'store_records', 'all'), getattr(exp, 'store_events', 'dat')
    if kind not in STORE_RECORDS:
        raise ValueError(f'store_records must be one of {STORE_RECORDS}, got {kind!r}')
    if events not in STORE_EVENTS:
        raise ValueError(f'store_events must be one of {STORE_EVENTS}, got {events!r}')
    if events == 'packed' and kind != 'windows':
        raise ValueError(f"store_events = 'packed' packs the records a window store keeps: it needs store_records = 'windows', got {kind!r}")
    cls = (Gen1PackedWindowStore if events == 'packed' else Gen1WindowStore) if kind == 'windows' else Gen1Store
    window = (exp.window * 1000, 0)
    made = (lambda store: store.trim()) if kind == 'windows' else (lambda store: store)
    ignore = tuple(getattr(exp, 'store_ignore', ()))        # recordings left out (the reference's ``dirs_to_ignore``); none unless the experiment names some

    def synthetic(device, shard):
        n_files, n_labels, n_events = getattr(exp, 'store_recordings', (4, 16, 50_000))
        size = exp.test_size if split == 'test' else exp.input_size
        sensor = (min(240, size[0]), min(304, size[1]))
        recs = synth_gen1_recordings(n_files, n_labels, n_events, sensor, num_classes=max(int(exp.num_classes), 1), seed=int(split == 'test'))
        return made(cls(recs, exp.Tl, window, device, sensor_hw=sensor, shard=shard))
    return _store_for(exp, '_dat_stores' if kind == 'all' else '_dat_packed_stores' if events == 'packed' else '_dat_window_stores',
                      split, device, lambda: _data_dirs(exp, split),
                      lambda dirs, device, shard: made(cls.from_directories(dirs, exp.Tl, window, device, ignore=ignore, shard=shard)), synthetic,
                      snapshot=lambda dirs, shard: ('dat_store', cls, dict(Tl=int(exp.Tl), window=window, sensor_hw=(240, 304), ignore=sorted(ignore),
                                                                           store_records=kind, store_events=events),
                                                    str(exp.data_dir), cls._source_files(dirs, ignore, shard)))


class _StoreDataset:
    """what the trainer and the evaluators ask of a dataset, over a store: length, ``sample_names``, ``class_names`` (the class indices
    as strings unless the class says otherwise), ``map_val`` without random augmentation"""
    map_val, random_aug = True, False

    def __init__(self, exp, store):
        self.exp, self.store, self.sample_names = exp, store, store.sample_names
        self.class_names = self._class_names()

    def _class_names(self):
        return [str(i) for i in range(self.exp.num_classes)]

    def __len__(self):
        return len(self.store)


class _StoreLoader:
    """The training loader over a store (``Gen1StoreLoader`` says what it does, on one rank and on N).  A class states: ``jitter`` of
    ``jitter_params``; ``permutes``: whether a sample's boxes are permuted -- where not, nothing is drawn for them and ``batches`` holds
    (indices, params) only; ``what``: its samples, in the message of a store smaller than a batch; ``Dataset``; ``make_store(exp)``: the
    store when none is given; ``check(exp)``: what it asks of the experiment (ValueError), before it looks at the store."""
    jitter, permutes, what, Dataset = .3, True, 'labels', _StoreDataset

    def __init__(self, exp, batch_size, store=None, seed=0, max_labels=50, rank=0, world=1):
        self.exp, self.batch_size, self.seed, self.max_labels = exp, batch_size, seed, max_labels
        self.check(exp)
        self.store = store if store is not None else self.make_store(exp)
        self._plan(rank, world)
        self.dataset = self.Dataset(exp, self.store)
        self.epoch = 0

    def check(self, exp):
        pass

    def _plan(self, rank, world):
        """``rank``, ``world``, ``sharded`` and ``iters`` of a training loader over ``self.store``"""
        self.rank, self.world = (int(rank), int(world)) if self.store.shard is None else self.store.shard
        if not 0 <= self.rank < self.world:
            raise ValueError(f'rank {rank} of a world of {world}')
        self.sharded = self.store.sharded
        if self.sharded:
            self.iters = _sharded_iters(self.store, self.batch_size, self.rank)
        else:
            self.iters = len(self.store) // (self.batch_size * self.world)
            assert self.iters >= 1, f'fewer {self.what} than one batch'

    def _epoch(self, epoch):
        """(random state, sample order, samples drawn per step, the rows of a step that this rank keeps) of an epoch"""
        if self.sharded:
            rs = _shard_state(self.seed, epoch, self.rank)
            return rs, self.store.owned_samples[rs.permutation(len(self.store.owned_samples))], self.batch_size, slice(None)
        rs = np.random.RandomState((self.seed * 1_000_003 + epoch) % (1 << 32))
        return rs, rs.permutation(len(self.store)), self.batch_size * self.world, slice(self.rank, None, self.world)

    def __len__(self):
        return self.iters

    def close_mosaic(self):
        pass

    def batches(self, epoch):
        """[(sample indices int64 [B], params int32 [B, 5], box permutations int32 [B, P])] of an epoch; P = the store's largest group (at
        least 1), a row of a smaller group is filled up with the identity.  A loader that does not permute: [(indices, params)]."""
        rs, order, drawn, keep = self._epoch(epoch)
        (H, W), (Hc, Wc) = self.store.sensor_hw, self.exp.input_size
        P = max(self.store.max_group_rows, 1)
        out = []
        for i in range(self.iters):
            idx = order[i * drawn:(i + 1) * drawn].astype(np.int64)
            par = np.empty((len(idx), 5), dtype=np.int32)
            perm = np.tile(np.arange(P, dtype=np.int32), (len(idx), 1))
            for b, s in enumerate(idx):
                par[b] = jitter_params(H, W, Hc, Wc, jitter=self.jitter, rng=rs)
                if self.permutes:
                    n = int(self.store.group_rows[s])
                    perm[b, :n] = rs.permutation(n)
            out.append(tuple(np.ascontiguousarray(a[keep]) for a in ((idx, par, perm) if self.permutes else (idx, par))))
        return out

    def __iter__(self):
        dev = self.store.device
        draws = self.batches(self.epoch)
        self.epoch += 1
        for batch in draws:
            self.store.check_owned(batch[0])
            idx, par, *perm = (torch.from_numpy(a).to(dev) for a in batch)      # (``perm``: one tensor, or none for a store whose ``targets`` takes none)
            yield self.store.frames(idx, par, self.exp), self.store.targets(idx, par, *perm, self.exp.input_size, self.max_labels)


class _StoreEvalLoader:
    """The evaluation loader over a store (``Gen1StoreEvalLoader`` says what it does).  A class states its ``Dataset`` and ``check(exp)``."""
    Dataset = _StoreDataset

    def __init__(self, exp, batch_size, indices, store, min_batches=0):
        self.exp, self.batch_size, self.indices, self.store, self.min_batches = exp, batch_size, list(indices), store, int(min_batches)
        self.check(exp)
        store.check_owned(self.indices)
        self.dataset = self.Dataset(exp, store)
        self.labels = {i: torch.from_numpy(store.raw_labels(i)) for i in set(self.indices)}

    def check(self, exp):
        pass

    def __len__(self):
        return max((len(self.indices) + self.batch_size - 1) // self.batch_size, self.min_batches)

    def _empty(self):
        """a batch without samples"""
        frames = torch.zeros((0, getattr(self.store, 'Tl', 1), self.exp.Tm, 2) + tuple(self.exp.test_size), device=self.store.device)
        return frames, [], (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)), torch.zeros(0, dtype=torch.int64)

    def __iter__(self):
        (H, W), (Hc, Wc) = self.store.sensor_hw, self.exp.test_size
        row = letterbox_params(H, W, Hc, Wc)
        for b in range(len(self)):
            ids = self.indices[b * self.batch_size:(b + 1) * self.batch_size]
            if not ids:
                yield self._empty()
                continue
            idx = torch.tensor(ids, dtype=torch.int64).to(self.store.device)
            frames = self.store.frames(idx, [row] * len(ids), self.exp, canvas_hw=(Hc, Wc))
            yield frames, [self.labels[i] for i in ids], (torch.full((len(ids),), H), torch.full((len(ids),), W)), torch.tensor(ids)


class Gen1StoreDataset(_StoreDataset):
    """``_StoreDataset`` over a ``Gen1Store``: the sample names carry the label time the Prophesee protocol reads"""


class Gen1StoreLoader(_StoreLoader):
    """Training loader of Gen1 from a ``Gen1Store``: iterable of (frames [B, Tl, Tm, 2, Hc, Wc] fp32 on the GPU, targets [B, 50, 5] rows
    (cls, cx, cy, w, h), zero padded).  An epoch is a permutation of the samples; per sample the draws come in the reference's order
    (get_random_data, gen1.py:485-511): ``jitter_params(..., jitter=.3)``, then the permutation of its boxes, ``rng.permutation(n)`` -- the
    order ``np.random.shuffle`` gives the rows under the same state.  ``batches(epoch)`` returns the draws of an epoch, a function of (seed,
    epoch) alone; a step uploads them -- sample indices, params, box permutations -- and everything else happens on the device
    (``store.frames``, ``store.targets``): no host read, no per-sample work.  ``store=None``: ``gen1_store_for(exp)``.

    On N ranks (``rank``, ``world``; ``batch_size`` is the per-rank batch b, the global batch is B = b * world):

    * over a store that holds everything (replica mode) the epoch is the single-process epoch of batch B, and a rank keeps rows
      ``rank::world`` of every batch: ``batches(e)[i]`` equals rows ``rank::world`` of ``Loader(exp, B, store, seed).batches(e)[i]``, array
      for array, and ``len(loader) == len(store) // B``.  The random state is consumed in the global order -- every rank computes the
      global draws and keeps its rows -- so the N rank batches of a step, interleaved, are the single-process batch with the same draw
      per sample: the reference's ``InfiniteSampler`` (``perm[rank::world]``) taken b at a time.
    * over a sharded store (``store.sharded``) an epoch is a permutation of ``store.owned_samples``, drawn -- with the per-sample draws, in
      the same order -- from ``_shard_state(seed, epoch, rank)``: a function of (seed, epoch, rank) alone that differs between ranks.
      ``len(loader)`` is the smallest owned count of any rank // b (``_sharded_iters``).  The rank is the store's (``store.shard``)
      where it has one.

    Before a step uploads its indices they are checked against ``store.owns`` on the host: IndexError for a sample whose records are
    not here."""

    Dataset = Gen1StoreDataset

    def check(self, exp):
        exp_aggregation(exp)

    def make_store(self, exp):
        return gen1_store_for(exp)


class Gen1StoreEvalLoader(_StoreEvalLoader):
    """Evaluation loader over a ``Gen1Store``: iterable of the tuple ``SyntheticEvalLoader`` yields -- ``(frames [B, Tl, Tm, 2, H, W] fp32
    on the GPU, labels [B][n, 5] rows (x, y, w, h, cls), (heights, widths), ids)``.  The frames go through the deterministic branch of
    get_random_data (``letterbox_params`` of the sensor on ``exp.test_size``); the labels are the raw float32 rows of the store
    (``Gen1Store.raw_labels``), prepared on the host once.  ``indices`` are this rank's samples; the last batch may be short.  An index
    whose records the store does not hold raises IndexError here, on the host.  ``min_batches``: the loader is at least that long;
    the batches behind the last sample are empty (B = 0: no frames, no labels, no ids) -- what the ranks of a sharded evaluation, which
    own different numbers of samples, are padded with where an evaluator meets the other ranks once per batch."""

    Dataset = Gen1StoreDataset

    def check(self, exp):
        exp_aggregation(exp)


# ------------------------------------------------------------------------------------------------ 1 Mpx from recordings resident in HBM
GEN4_REP_NAME = 'stacked_histogram_dt=50_nbins=10'        # RVTGEN4Dataset's default ``rep_name``
GEN4_LABEL_FIELDS = ('t', 'x', 'y', 'w', 'h', 'class_id', 'class_confidence')        # _str2idx, rvt_gen4.py:34-42
GEN4_BBOX_DTYPE = np.dtype([('t', '<u8'), ('x', '<f4'), ('y', '<f4'), ('w', '<f4'), ('h', '<f4'), ('class_id', 'u1'), ('class_confidence', '<f4')])


def synth_gen4_recordings(n_files, representations, sensor_hw=(360, 640), nbins=10, num_classes=3, seed=0):
    """``n_files`` seeded recordings ``(name, representations, objframe_idx_2_repr_idx, label_rows, objframe_idx_2_label_idx, label_times)``
    as ``Gen4Store`` takes them, so that the store and its loaders run without a dataset.  Representations: u8 [representations, 2 * nbins,
    H, W], Poisson(0.03) clamped to 255 (the histograms of ``SyntheticStackedHistLoader.store``), 50 ms apart.  Object frames: at
    representations 1, 3, 4, 6, 7, 9, ... (two of every three; the first is younger than a sample of three slices), label time = the end of
    the representation, the first one at 450 ms.  Object frame k carries 3, 0, 1, 2 boxes for k % 4 = 0, 1, 2, 3, some of them across the
    borders; the rows (``GEN4_BBOX_DTYPE``) are in the coordinates of the stored labels, twice the sensor's (``down_sample_factor`` 2)."""
    H, W = sensor_hw
    out = []
    for f in range(n_files):
        rng = np.random.default_rng([seed, f])
        reps = np.minimum(rng.poisson(0.03, size=(representations, 2 * nbins, H, W)), 255).astype(np.uint8)
        obj2repr = np.array([i for i in range(1, representations) if i % 3 != 2], dtype=np.int64)
        times = 400_000 + 50_000 * (obj2repr + 1)
        rows, first = [], []
        for k, t in enumerate(times):
            first.append(len(rows))
            for _ in range((3, 0, 1, 2)[k % 4]):
                bw, bh = rng.uniform(0.15, 0.4) * 2 * W, rng.uniform(0.15, 0.4) * 2 * H
                bx, by = rng.uniform(-0.1, 0.9) * 2 * W, rng.uniform(-0.1, 0.9) * 2 * H
                rows.append((int(t), bx, by, bw, bh, int(rng.integers(0, max(num_classes, 1))), 1.0))
        out.append((f'synthetic_{seed}_{f:03d}', reps, obj2repr, np.array(rows, dtype=GEN4_BBOX_DTYPE), np.asarray(first, dtype=np.int64),
                    times.astype(np.int64)))
    return out


def _h5_representations(rep_dir):
    """``data`` of ``<rep_dir>/event_representations_ds2_nearest.h5``, left open: the file RVTGEN4Dataset.generate_slices reads
    (rvt_gen4.py:118-119)"""
    import os
    try:
        import h5py
    except ImportError as e:
        raise ImportError('reading event_representations_ds2_nearest.h5 needs h5py, which is not installed; pass read_representations= (a '
                          'function of the representation directory that returns something that slices to u8 [r, 2 * nbins, H, W])') from e
    return h5py.File(os.path.join(rep_dir, 'event_representations_ds2_nearest.h5'), 'r')['data']


class Gen4Store(_Store):
    """1 Mpx (Gen4, RVT pre-processed) recordings and their labels resident on the device: what RVTGEN4Dataset keeps on disk and in host lists
    (rvt_gen4.py:93-97, 365-409), as tables that the kernels index.  ``recordings``: a list of ``(name, representations,
    objframe_idx_2_repr_idx, label_rows, objframe_idx_2_label_idx, label_times)`` -- ``representations`` is anything that has a length and
    slices to u8 [r, 2 * nbins, H, W] (a numpy array, a memmap, an h5py dataset); ``label_rows`` the structured ``labels`` array of
    ``labels.npz`` (fields ``GEN4_LABEL_FIELDS``) or float rows [L, 7] in that order; ``label_times`` one time per object frame (another
    length raises ValueError, as the reference asserts).  ``num_slice``: representations per sample -- the reference's ``num_slice`` slice
    argument, ``exp.Tm`` on this project's 1 Mpx path.

    The model only ever sees the bin sums (generate_slices with ``'event_sum'``, rvt_gen4.py:120-122), so the sums are what is kept:
    ``sums`` ``torch.uint16`` [R, 2, H, W], allocated once at its final size; every recording is read ``chunk`` representations at a time,
    uploaded, and summed into its place by ``ops.stacked_hist_bin_sums`` -- exact, 2 bytes per pixel and polarity where the representations
    hold ``nbins``, and the u8 form never exists whole on the device.  Built on the host and uploaded once: ``rep_offsets`` int64 [F + 1]
    (index in ``sums`` of every recording's first representation), ``group_first`` int64 [G] (``rvt_first_index``: the representation that
    feeds slice 0 of the sample; below ``group_lo`` for a young sequence), ``group_lo`` int64 [G] (the offset of the sample's recording),
    ``boxes`` float32 [L, 5] rows (x1, y1, x2, y2, class) -- ``gen4_raw_boxes(gen4_rescale_labels(rows, down_sample_factor, sensor_hw))`` per
    object frame, cut as extract_labels cuts the rows (the last frame open-ended) -- and ``group_start`` int64 [G + 1].  On the host:
    ``sample_names`` ``<name>_n<num_slice>_a<label time>`` (get_sample_resp, rvt_gen4.py:246-248), ``group_rows``, ``max_group_rows`` and
    numpy copies of the tables (``host``).  Every object frame is a sample, one without boxes too (the reference's ``__len__`` counts object
    frames); the flat sample index is recordings in the order given, then object frames in order (resolve_index, rvt_gen4.py:296-300).

    ``device='cpu'`` builds the tables and leaves ``sums`` None: the representations are only measured, there is no summing on the host.

    On N ranks a store holds the labels of every recording and the bin sums of its own: ``owned`` (a collection of recording names, None
    = all) or ``shard=(rank, world)`` (``shard_recordings`` by ``len(representations)``).  ``rep_offsets``, ``group_first`` and
    ``group_lo`` stay in the coordinates of the whole dataset -- with ``boxes``, ``group_start``, ``sample_names``, the flat sample index,
    ``raw_labels``, ``targets`` and the length they are the same on every rank and the same as the unsharded store's; a recording that
    is not owned may pass None as its ``representations`` and is never touched (it then counts ``objframe_idx_2_repr_idx[-1] + 1``
    representations, 0 without object frames: the weight ``from_directories`` gives it).  What ``sums`` holds is described by
    ``held_offsets`` (host, int64 [F + 1]: a recording that is not owned has a zero-length area) and the device tables ``held_first`` /
    ``held_lo`` int64 [G] that ``frames`` gathers: ``group_first`` / ``group_lo`` moved to the recording's place in ``sums``; a sample that
    is not owned has ``held_first = -num_slice``, ``held_lo = 0``: every slice lies in front of its recording and is zero.  Without
    ``owned`` / ``shard`` the held tables are the group tables themselves.  ``owned_samples``, ``owns``, ``shard``, ``sample_rank``: see
    ``_Store``."""
    _snapshot_fields = dict(scalars=('num_slice', 'sensor_hw', 'nbins', 'down_sample_factor'), lists=(), host=('held_offsets',), device=('sums',))

    def __init__(self, recordings, num_slice, device, down_sample_factor=2, sensor_hw=(360, 640), nbins=10, chunk=64, owned=None, shard=None):
        self.num_slice, self.sensor_hw, self.nbins = int(num_slice), (int(sensor_hw[0]), int(sensor_hw[1])), int(nbins)
        self.down_sample_factor = down_sample_factor
        self.names, self.sample_names = [], []
        H, W = self.sensor_hw
        reps, rep_offsets, boxes, group_start, group_first, group_lo = [], [0], [], [0], [], []
        held_offsets, group_file = [0], []
        if shard is not None:
            recordings = list(recordings)
        owned, ranks = _memory_plan(recordings, lambda r: r[0], lambda r: r[1], shard, owned)
        for name, rep, obj2repr, rows, obj2label, label_times in recordings:
            obj2repr, obj2label = np.asarray(obj2repr, dtype=np.int64), np.asarray(obj2label, dtype=np.int64)
            mine = owned is None or name in owned
            if not mine:                                        # labels only: the representations are not looked at beyond their number
                n_rep = len(rep) if rep is not None else (int(obj2repr[-1]) + 1 if len(obj2repr) else 0)
                rep = np.zeros((0, 2 * self.nbins, H, W), dtype=np.uint8)
            elif tuple(rep.shape[1:]) != (2 * self.nbins, H, W):
                raise ValueError(f'{name}: representations of shape {tuple(rep.shape)}, expected [r, {2 * self.nbins}, {H}, {W}]')
            else:
                n_rep = len(rep)
            if len(label_times) != len(obj2label):
                raise ValueError(f'{name}: {len(label_times)} label times for {len(obj2label)} object frames')
            if getattr(rows, 'dtype', None) is not None and rows.dtype.names:
                rows = np.stack([rows[k].astype(np.float32) for k in GEN4_LABEL_FIELDS], axis=-1).reshape(-1, 7)
            rows = np.asarray(rows, dtype=np.float32).reshape(-1, 7)
            self.names.append(name)
            offset = rep_offsets[-1]
            reps.append(rep)
            rep_offsets.append(offset + n_rep)
            held_offsets.append(held_offsets[-1] + len(rep))
            group_file += [len(self.names) - 1] * len(obj2label)
            ends = np.r_[obj2label[1:], len(rows)]
            for k, (a, b) in enumerate(zip(obj2label, ends)):
                box = gen4_raw_boxes(gen4_rescale_labels(rows[a:b], down_sample_factor, self.sensor_hw))
                boxes.append(box.astype(np.float32).reshape(-1, 5))
                group_start.append(group_start[-1] + len(box))
                group_first.append(int(rvt_first_index(obj2repr, k, self.num_slice, offset)))
                group_lo.append(offset)
                self.sample_names.append(f'{name}_n{self.num_slice}_a{int(label_times[k])}')
        self.device = torch.device(device)
        self._set_tables(dict(rep_offsets=np.asarray(rep_offsets, dtype=np.int64), group_first=np.asarray(group_first, dtype=np.int64),
                              group_lo=np.asarray(group_lo, dtype=np.int64),
                              boxes=np.concatenate(boxes).astype(np.float32) if boxes else np.zeros((0, 5), np.float32),
                              group_start=np.asarray(group_start, dtype=np.int64)))
        self.group_file = group_file = np.asarray(group_file, dtype=np.int64)                # (host: the recording of every sample)
        self._set_owners(self.names, group_file, owned, ranks, shard)
        self.held_offsets = np.asarray(held_offsets, dtype=np.int64)
        self._set_held()
        self.sums = None
        if self.device.type != 'cpu':
            self._sum_recordings(reps, held_offsets, int(chunk))

    def _set_held(self):
        """``held_first`` / ``held_lo`` from the group tables, ``held_offsets``, ``group_file`` and the owners"""
        self.held_first, self.held_lo = self.group_first, self.group_lo
        if self.sharded:
            move = (self.held_offsets[:-1] - self.host['rep_offsets'][:-1])[self.group_file]
            first = np.where(self._sample_owned, self.host['group_first'] + move, -self.num_slice)
            lo = np.where(self._sample_owned, self.host['group_lo'] + move, 0)
            self.held_first, self.held_lo = (torch.from_numpy(v.astype(np.int64)).to(self.device) for v in (first, lo))

    def _loaded(self):
        self.group_file = self._owner_args[1]
        self._set_held()

    def _sum_recordings(self, reps, held_offsets, chunk):
        """the device side of the build: ``sums`` at its final size, every recording uploaded ``chunk`` representations at a time and summed
        into its place (``reps``: the representations of every recording, empty where not owned; ``held_offsets``: their places)"""
        H, W = self.sensor_hw
        self.sums = torch.empty((held_offsets[-1], 2, H, W), dtype=torch.uint16, device=self.device)
        for rep, offset in zip(reps, held_offsets):
            for a in range(0, len(rep), chunk):
                part = torch.from_numpy(np.ascontiguousarray(rep[a:a + chunk], dtype=np.uint8)).to(self.device)
                ops.stacked_hist_bin_sums(part, self.nbins, out=self.sums[offset + a:offset + a + part.shape[0]])

    @classmethod
    def from_directories(cls, paths, num_slice, device, down_sample_factor=2, sensor_hw=(360, 640), nbins=10, chunk=64, rep_name=GEN4_REP_NAME,
                         read_representations=None, shard=None):
        """the streams of the directories ``paths`` (extract_labels, rvt_gen4.py:389-407), every directory in sorted order (the reference
        takes them as ``os.listdir`` gives them): ``<stream>/labels_v2/labels.npz`` (``labels``, ``objframe_idx_2_label_idx``) and
        ``timestamps_us.npy``, ``<stream>/event_representations_v2/<rep_name>/objframe_idx_2_repr_idx.npy``, and the representations from
        ``read_representations(rep_dir)``.  Its default opens ``event_representations_ds2_nearest.h5`` with ``h5py`` (imported there; an
        ImportError that names ``h5py`` and this argument when it is missing) and returns its ``data``.  ``h5py`` is not among this
        project's requirements: that default is the one line of the store no test reaches.  ``shard=(rank, world)``: every stream is
        listed and its label files are read; a stream weighs the last entry of its ``objframe_idx_2_repr_idx.npy`` + 1 (0 for an empty
        file) -- the representations that its samples can reach, known without opening them --, and ``read_representations`` is called for
        the streams ``shard_recordings`` gives to ``rank`` only."""
        import os
        read = read_representations if read_representations is not None else _h5_representations
        listed = []
        for stream, label_dir, rep_dir in cls._listed(paths, rep_name):
            labels = np.load(os.path.join(label_dir, 'labels.npz'))
            listed.append((stream, rep_dir, np.load(os.path.join(rep_dir, 'objframe_idx_2_repr_idx.npy')), labels['labels'],
                           labels['objframe_idx_2_label_idx'], np.load(os.path.join(label_dir, 'timestamps_us.npy'))))
        owned, ranks = _shard_plan([r[0] for r in listed], [int(r[2][-1]) + 1 if len(r[2]) else 0 for r in listed], shard, None)
        recs = [(r[0], read(r[1]) if owned is None or r[0] in owned else None) + r[2:] for r in listed]
        store = cls(recs, num_slice, device, down_sample_factor=down_sample_factor, sensor_hw=sensor_hw, nbins=nbins, chunk=chunk, owned=owned)
        store._adopt(shard, ranks)
        return store

    @staticmethod
    def _listed(paths, rep_name=GEN4_REP_NAME):
        """[(stream, its label directory, its representation directory)] in the order of ``from_directories``; nothing is read"""
        import os
        return [(stream, os.path.join(path, stream, 'labels_v2'), os.path.join(path, stream, 'event_representations_v2', rep_name))
                for path in ([paths] if isinstance(paths, str) else paths) for stream in sorted(os.listdir(path))]

    @classmethod
    def _source_files(cls, paths, rep_name=GEN4_REP_NAME):
        """the files ``from_directories`` can open, from the listing alone: of every stream the two label files and every file of its
        representation directory (the index and whatever ``read_representations`` reads) -- of every stream on every rank, since which
        streams a shard owns is known only once their index files have been read"""
        import os
        out = []
        for _, label_dir, rep_dir in cls._listed(paths, rep_name):
            out += [os.path.join(label_dir, 'labels.npz'), os.path.join(label_dir, 'timestamps_us.npy')]
            out += [os.path.join(rep_dir, fn) for fn in sorted(os.listdir(rep_dir)) if os.path.isfile(os.path.join(rep_dir, fn))]
        return out

    def frames(self, sample_idx, params, exp, canvas_hw=None):
        """model input [B, 1, num_slice, 2, Hc, Wc] fp32 of the samples ``sample_idx`` (int64 [B] on the device): ``group_first`` and
        ``group_lo`` gathered on the device, then ``ops.count_store_frames``; ``params``: (nw, nh, dx, dy, flip) per sample, None = the
        sensor unscaled at the top left; ``canvas_hw``: ``exp.input_size`` unless given.  ``exp.Tm`` must be the store's ``num_slice``;
        ``exp.aggregation`` is not consulted (the representations are histograms already).  Nothing is read back (graph-capturable).
        Precondition: the store holds the bin sums of every sample asked for (``owns``; the loaders check their indices on the host before
        they upload them) -- a sample that is not owned comes out as zero frames, silently.  ``group_first`` / ``group_lo`` in the text
        above are ``held_first`` / ``held_lo``, the same tables unless the store is sharded."""
        if getattr(exp, 'Tm', self.num_slice) != self.num_slice:
            raise ValueError(f'the store was built for {self.num_slice} slices per sample, the experiment asks for Tm = {exp.Tm}')
        Hc, Wc = canvas_hw if canvas_hw is not None else exp.input_size
        return self._frames_from(self.held_first[sample_idx], self.held_lo[sample_idx], Hc, Wc,
                                 None if params is None else params_on(params, self.device))

    def _frames_from(self, first, lo, Hc, Wc, params):
        """the frame operator of this store's form on gathered indices"""
        return ops.count_store_frames(self.sums, first, self.num_slice, Hc, Wc, lo=lo, params=params)


class Gen4PackedStore(Gen4Store):
    """``Gen4Store`` with the bin sums in packed rows (include/eas_hip.h states the format): a row -- one sensor row of one polarity of one
    representation -- is cut into groups of 16 pixels; an all-zero group stores nothing, a group whose sums are all at most 255 stores 16
    bytes, any other its sixteen u16.  ``rows`` int64 [R, 2, H, 3] = (nz, wide, offset) per row, ``payload`` uint8 [used_bytes]; ``sums`` stays
    None.  The frames are bit-identical to the parent's (``ops.packed_store_frames``: the band kernel decodes a group where it stages it);
    labels, names, ``targets``, ``raw_labels``, ``owned`` / ``shard`` and ``from_directories`` are the parent's.

    The build, per chunk of ``chunk`` representations: upload, ``ops.stacked_hist_bin_sums`` into a chunk-sized scratch,
    ``ops.count_rows_pack`` into the arena at the position reached -- the full u16 form never exists on the device.  The arena is allocated
    once, ``capacity_bytes`` (None: the smaller of the u16 size of what the store holds -- rows counted in whole groups, which no packing
    exceeds -- and 0.8 of the free device memory); recordings that need more raise ValueError naming the bytes needed, after everything was
    measured.  ``used_bytes``: what the rows take; ``nbytes``: table + used payload; ``trim()`` gives the rest of the arena back.  A sensor
    wider than 1024 pixels raises ValueError (64 groups per row).  ``device='cpu'`` builds the tables and leaves ``rows`` / ``payload`` None."""
    _snapshot_fields = dict(Gen4Store._snapshot_fields, scalars=Gen4Store._snapshot_fields['scalars'] + ('used_bytes',), device=('rows', 'payload'))

    def _loaded(self):
        super()._loaded()
        self.sums, self.capacity_bytes = None, self.used_bytes

    def __init__(self, recordings, num_slice, device, down_sample_factor=2, sensor_hw=(360, 640), nbins=10, chunk=64, owned=None, shard=None,
                 capacity_bytes=None):
        if int(sensor_hw[1]) > ops.PACKED_MAX_W:
            raise ValueError(f'packed rows hold at most 64 groups of 16 pixels: a sensor of width {int(sensor_hw[1])} > {ops.PACKED_MAX_W}')
        self.capacity_bytes = None if capacity_bytes is None else int(capacity_bytes)
        self.rows, self.payload, self.used_bytes = None, None, 0
        super().__init__(recordings, num_slice, device, down_sample_factor=down_sample_factor, sensor_hw=sensor_hw, nbins=nbins, chunk=chunk,
                         owned=owned, shard=shard)

    def _sum_recordings(self, reps, held_offsets, chunk):
        H, W = self.sensor_hw
        R = int(held_offsets[-1])
        if self.capacity_bytes is None:
            u16_bytes = R * 2 * H * ((W + 15) // 16) * 32
            self.capacity_bytes = min(u16_bytes, int(0.8 * torch.cuda.mem_get_info(self.device)[0]))
        arena = self._arena = _Arena(max(self.capacity_bytes, 0), 16, self.device)
        self.capacity_bytes = arena.capacity_bytes
        self.rows = torch.empty((R, 2, H, 3), dtype=torch.int64, device=self.device)
        scratch = torch.empty((min(chunk, max([len(r) for r in reps], default=0)), 2, H, W), dtype=torch.uint16, device=self.device)
        for rep, offset in zip(reps, held_offsets):
            for a in range(0, len(rep), chunk):
                part = torch.from_numpy(np.ascontiguousarray(rep[a:a + chunk], dtype=np.uint8)).to(self.device)
                n = part.shape[0]
                sums = ops.stacked_hist_bin_sums(part, self.nbins, out=scratch[:n])
                del part
                try:
                    took = ops.count_rows_pack(sums, self.rows[offset + a:offset + a + n], arena.buf, arena.units, dry_run=arena.full)
                except ops.PackedArenaFull as e:                # too small: go on measuring, store nothing more
                    took, arena.full = e.units, True
                arena.place(took)
        if arena.full:
            self.rows = None
        self.payload = arena.close('packed rows')
        self.used_bytes = arena.used_bytes

    @property
    def nbytes(self):
        """bytes of the row table and of the payload in use"""
        return self.rows.numel() * 8 + self.used_bytes

    def trim(self):
        """give back what the arena does not use: ``payload`` is reallocated at its size (``_Arena.trim``); a store that ``load_store``
        made has nothing to give back"""
        if getattr(self, '_arena', None) is None:
            return self
        self.payload, self.capacity_bytes = self._arena.trim(), self._arena.used_bytes
        return self

    def unpacked(self, a, b):
        """``torch.uint16`` [b - a, 2, H, W]: the bin sums of the held representations ``a`` .. ``b`` in the parent's form"""
        return ops.count_rows_unpack(self.rows[a:b], self.payload, self.sensor_hw[1])

    def _frames_from(self, first, lo, Hc, Wc, params):
        """``frames`` is the parent's: ``held_first`` / ``held_lo`` gathered on the device, then ``ops.packed_store_frames`` in place of
        ``ops.count_store_frames`` (nothing read back, graph-capturable)"""
        return ops.packed_store_frames(self.rows, self.payload, first, self.num_slice, Hc, Wc, lo=lo, params=params, W=self.sensor_hw[1])


STORE_SUMS = ('u16', 'packed')              # ``exp.store_sums``: the bin sums as uint16 planes (Gen4Store) / in packed rows (Gen4PackedStore)


def hist_store_for(exp, split='train', device=None):
    """The store of an experiment with ``train_input = 'hist_store'``: ``Gen4Store.from_directories`` over ``exp.data_dir``/train + /val
    (``split='test'``: /test) when those directories exist, seeded synthetic recordings otherwise (``exp.store_recordings`` = (files,
    representations per file), default (2, 24); the sensor is the downsampled 1 Mpx camera's, or the canvas where that is smaller).
    ``num_slice`` is ``exp.Tm``; ``exp.nbins`` (default 10) and ``exp.down_sample_factor`` (default 2) are read where present.
    ``exp.store_shard`` = ``'recordings'``: the store of this rank.  ``exp.store_sums`` (default ``'u16'``) = ``'packed'``: a
    ``Gen4PackedStore``; any other value raises ValueError.  Kept on the experiment: one store per (split, rank, world, store_shard,
    store_sums)."""
    kind = getattr(exp, 'store_sums', 'u16')
    if kind not in STORE_SUMS:
        raise ValueError(f'store_sums must be one of {STORE_SUMS}, got {kind!r}')
    cls = Gen4PackedStore if kind == 'packed' else Gen4Store
    nbins, factor = int(getattr(exp, 'nbins', 10)), getattr(exp, 'down_sample_factor', 2)

    def synthetic(device, shard):
        n_files, n_reps = getattr(exp, 'store_recordings', (2, 24))[:2]
        size = exp.test_size if split == 'test' else exp.input_size
        sensor = (min(360, size[0]), min(640, size[1]))
        recs = synth_gen4_recordings(n_files, n_reps, sensor, nbins, num_classes=max(int(exp.num_classes), 1), seed=int(split == 'test'))
        return cls(recs, exp.Tm, device, down_sample_factor=2, sensor_hw=sensor, nbins=nbins, shard=shard)
    return _store_for(exp, '_hist_stores', split, device, lambda: _data_dirs(exp, split),
                      lambda dirs, device, shard: cls.from_directories(dirs, exp.Tm, device, down_sample_factor=factor, nbins=nbins, shard=shard),
                      synthetic, more=(kind,),
                      snapshot=lambda dirs, shard: ('hist_store', cls, dict(num_slice=int(exp.Tm), nbins=nbins, down_sample_factor=factor,
                                                                            sensor_hw=(360, 640), rep_name=GEN4_REP_NAME, store_sums=kind),
                                                    str(exp.data_dir), cls._source_files(dirs)))


class Gen4StoreDataset(_StoreDataset):
    """``_StoreDataset`` over a ``Gen4Store``: the sample names carry the label time, as Gen1's do"""


class Gen4StoreLoader(_StoreLoader):
    """Training loader of the 1 Mpx path from a ``Gen4Store``: iterable of (frames [B, 1, Tm, 2, Hc, Wc] fp32 on the GPU, targets [B, 50, 5]
    rows (cls, cx, cy, w, h), zero padded).  The epochs, the draws and the step are ``Gen1StoreLoader``'s: an epoch is a permutation of the
    samples; per sample ``jitter_params(..., jitter=.3)``, then ``rng.permutation(n)`` of its boxes, in get_random_data's order
    (rvt_gen4.py:562-588); ``batches(epoch)`` is a function of (seed, epoch); a step uploads indices, params and permutations and nothing
    else.  ``exp.aggregation`` is not consulted, as in ``SyntheticStackedHistLoader``.  ``store=None``: ``hist_store_for(exp)``.  ``rank``,
    ``world`` and a sharded store: as in ``Gen1StoreLoader``."""

    Dataset = Gen4StoreDataset

    def make_store(self, exp):
        return hist_store_for(exp)


class Gen4StoreEvalLoader(_StoreEvalLoader):
    """Evaluation loader over a ``Gen4Store``: iterable of the tuple ``Gen1StoreEvalLoader`` yields -- ``(frames [B, 1, Tm, 2, H, W] fp32 on
    the GPU, labels [B][n, 5] rows (x, y, w, h, cls), (heights, widths), ids)`` -- by that loader's own loop: ``letterbox_params`` of the
    sensor on ``exp.test_size``, the raw float32 rows of ``Gen4Store.raw_labels``, the sensor's sizes.  ``exp.aggregation`` is not
    consulted."""

    Dataset = Gen4StoreDataset


# ------------------------------------------------------------------------------------------------ N-Caltech101 from recordings resident in HBM
NCALTECH_BACKGROUND = 'BACKGROUND_Google'          # the class the reference leaves out (ncaltech.py:48-51, 129-134)


def parse_ncaltech_annotation(buf):
    """``(x1, y1, x2, y2)`` of an N-Caltech101 ``annotation_*.bin`` image (bytes or a uint8 array), as NCaltech.read_annotation finds them
    (ncaltech.py:107-127): two int16 (rows, cols), the box contour as rows * cols int16 in column-major order, and the minimum / maximum of
    its rows 0 (x) and 1 (y).  The object contour behind it is not looked at."""
    raw = buf.tobytes() if isinstance(buf, np.ndarray) else bytes(buf)
    rows, cols = (int(v) for v in np.frombuffer(raw, dtype='<i2', count=2))
    contour = np.frombuffer(raw, dtype='<i2', count=rows * cols, offset=4).reshape((rows, cols), order='F')
    return int(contour[0].min()), int(contour[1].min()), int(contour[0].max()), int(contour[1].max())


def encode_ncaltech_annotation(x1, y1, x2, y2, contour=((0, 0),)):
    """The inverse of ``parse_ncaltech_annotation``, numpy uint8: a 2 x 5 box contour -- the rectangle's corners, closed, as the dataset's
    files hold it -- and the object contour ``contour`` (points (x, y)) behind it."""
    box = np.array([[x1, x2, x2, x1, x1], [y1, y1, y2, y2, y1]], dtype='<i2')
    obj = np.asarray(contour, dtype='<i2').reshape(-1, 2).T
    parts = [np.array(a.shape, dtype='<i2').view(np.uint8) for a in (box, obj)]
    return np.concatenate([parts[0], box.reshape(-1, order='F').view(np.uint8), parts[1], obj.reshape(-1, order='F').view(np.uint8)])


def synth_ncaltech_recordings(n_files, n_events, sensor_hw=(180, 240), n_classes=3, span_us=300_000, seed=0):
    """``n_files`` seeded recordings ``(class_name, stem, atis_bytes uint8, annotation_bytes uint8)`` as ``NCaltechStore`` takes them, so that
    the store and its loaders run without a dataset.  Recording f holds between ``n_events`` / 2 and ``n_events`` events -- ``t`` sorted uniform
    over ``span_us``, ``x``, ``y`` uniform on the sensor, ``p`` Bernoulli(0.5) --, an overflow record in front of the first event of every further
    65536 us (``encode_atis``), class ``f % n_classes`` and one box: inside the sensor, or (every fourth) across its right and lower border."""
    H, W = sensor_hw
    out = []
    for f in range(n_files):
        rng = np.random.default_rng([seed, f])
        n = int(rng.integers(n_events // 2, n_events + 1))
        t = np.sort(rng.integers(0, span_us, size=n, dtype=np.int64))
        x, y = rng.integers(0, W, size=n), rng.integers(0, H, size=n)
        p = (rng.random(n) < 0.5).astype(np.int64)
        marks = np.arange(1, span_us // 65536 + 1) * 65536
        bw, bh = int(rng.uniform(0.3, 0.6) * W), int(rng.uniform(0.3, 0.6) * H)
        bx, by = (W - bw // 2, H - bh // 2) if f % 4 == 3 else (int(rng.integers(0, W - bw)), int(rng.integers(0, H - bh)))
        out.append((f'class_{f % n_classes:03d}', f'image_{f:04d}', encode_atis(t, x, y, p, overflow_before=np.searchsorted(t, marks)),
                    encode_ncaltech_annotation(bx, by, bx + bw, by + bh)))
    return out


class NCaltechStore(_Store):
    """N-Caltech101 recordings and their boxes resident on the device: what NCaltech keeps on disk (ncaltech.py:43-61, 172-178), as tables that
    the kernels index.  ``recordings``: a list of ``(class_name, stem, atis_bytes, annotation_bytes)`` -- the byte images of
    ``Caltech101/<class>/<stem>.bin`` and its ``annotation`` file; recordings of ``BACKGROUND_Google`` are left out.  ``Tl``: macro slices per
    sample (the reference's ``num_slice``); ``window`` = (lo, hi) in us relative to the recording's last event, or None.

    Built once on the host and uploaded once: ``records`` uint8 (the recordings back to back), ``file_offsets`` int64 [F + 1] (record
    indices), ``index`` (``ops.atis_store_index(records)``, the buffer's overflow prefix: two launches over the store, never again), ``boxes``
    float32 [F, 5] rows (x1, y1, x2, y2, class) (``raw_bboxes``, ncaltech.py:176-177) and ``group_start`` = arange(F + 1): one box per
    sample.  On the host: ``sample_names`` ``<class>-<stem>`` (ncaltech.py:59, 194), ``class_names`` (given, else the sorted names of the
    recordings' classes), ``max_file_records`` and numpy copies of the tables (``host``).  The flat sample index is the recording's.

    On N ranks a store holds the boxes of every recording and the records of its own: ``owned`` (a collection of sample names
    ``<class>-<stem>``, None = all) or ``shard=(rank, world)`` (``shard_recordings`` by ``len(atis_bytes)``).  A recording that is not
    owned contributes its box, its name and a zero-length area to ``records`` / ``file_offsets``; its ``atis_bytes`` may be None and is
    never touched.  ``boxes``, ``group_start``, ``sample_names``, ``class_names``, ``raw_labels``, ``targets`` and the length are the same
    on every rank and the same as the unsharded store's; ``max_file_records`` is that of the owned recordings.  ``owned_samples``,
    ``owns``, ``shard``, ``sample_rank``: see ``_Store``."""
    _snapshot_fields = dict(scalars=('Tl', 'window', 'sensor_hw', 'max_file_records'), lists=('class_names',), host=(), device=('records', 'index'))

    def __init__(self, recordings, Tl, window, device, class_names=None, sensor_hw=(180, 240), owned=None, shard=None):
        self.Tl, self.sensor_hw = int(Tl), (int(sensor_hw[0]), int(sensor_hw[1]))
        self.window = None if window is None else (int(window[0]), int(window[1]))
        recordings = [r for r in recordings if r[0] != NCALTECH_BACKGROUND]
        owned, ranks = _memory_plan(recordings, lambda r: f'{r[0]}-{r[1]}', lambda r: r[2], shard, owned)
        if class_names is None:
            class_names = sorted({r[0] for r in recordings})
        self.class_names = list(class_names)
        name_to_idx = {name: i for i, name in enumerate(self.class_names)}
        self.sample_names = []
        areas, file_offsets, boxes = [], [0], []
        for cls, stem, rec, ann in recordings:
            if owned is not None and f'{cls}-{stem}' not in owned:
                rec = b''                                       # labels only: the recording is not looked at
            buf = np.frombuffer(rec, dtype=np.uint8) if isinstance(rec, (bytes, bytearray, memoryview)) else np.asarray(rec, dtype=np.uint8)
            if len(buf) % 5 != 0:
                raise ValueError(f'{cls}/{stem}: not an ATIS recording of 5-byte records ({len(buf)} bytes)')
            self.sample_names.append(f'{cls}-{stem}')
            areas.append(buf)
            file_offsets.append(file_offsets[-1] + len(buf) // 5)
            boxes.append(parse_ncaltech_annotation(ann) + (name_to_idx[cls],))
        F = len(self.sample_names)
        self.device = torch.device(device)
        self.records = torch.from_numpy(np.concatenate(areas) if areas else np.zeros(0, np.uint8)).to(self.device)
        self._set_tables(dict(file_offsets=np.asarray(file_offsets, dtype=np.int64), boxes=np.asarray(boxes, dtype=np.float32).reshape(F, 5),
                              group_start=np.arange(F + 1, dtype=np.int64)))
        self.max_file_records = int(np.diff(self.host['file_offsets']).max()) if F else 0
        self._set_owners(self.sample_names, np.arange(F), owned, ranks, shard)             # a recording is a sample
        # a store kept on the host is its tables only (names, boxes, offsets: what needs no GPU); the operators refuse its tensors
        self.index = ops.atis_store_index(self.records) if self.device.type == 'cuda' else None

    @classmethod
    def from_directory(cls, root, split, Tl, window, device, class_names=None, sensor_hw=(180, 240), shard=None, read_bin=None):
        """the recordings of ``<root>/<split>.txt`` -- ``data_path label_path`` per line, relative to ``root``; lines that name
        ``BACKGROUND_Google`` are dropped (ncaltech.py:48-51) --, read with ``numpy.fromfile``.  The class of a sample is the directory of its
        label file, its stem the data file's name up to the first dot.  ``class_names=None``: the sorted directory names of
        ``<root>/Caltech101`` without ``BACKGROUND_Google`` (ncaltech.py:129-134).  ``shard=(rank, world)``: every line is listed and every
        annotation read; a recording weighs the size of its ``.bin`` (``os.path.getsize``), and only the recordings ``shard_recordings``
        gives to ``rank`` are read.  ``read_bin(path)``: the reader of a recording (default ``numpy.fromfile(path, dtype=numpy.uint8)``)."""
        read_bin = read_bin if read_bin is not None else (lambda p: np.fromfile(p, dtype=np.uint8))
        if class_names is None:
            class_names = cls._listed_classes(root)
        listed, names, owned, ranks = cls._listed(root, split, shard)
        listed = [(c, stem, path, np.fromfile(label, dtype=np.uint8)) for c, stem, path, label in listed]
        recs = [(c, stem, read_bin(path) if owned is None or n in owned else None, ann) for n, (c, stem, path, ann) in zip(names, listed)]
        store = cls(recs, Tl, window, device, class_names=class_names, sensor_hw=sensor_hw, owned=owned)
        store._adopt(shard, ranks)
        return store

    @staticmethod
    def _listed_classes(root):
        import os
        return [n.strip() for n in sorted(os.listdir(os.path.join(root, 'Caltech101'))) if NCALTECH_BACKGROUND not in n]

    @staticmethod
    def _listed(root, split, shard):
        """([(class, stem, path of the recording, path of its annotation)] of ``<root>/<split>.txt`` in its order, their sample names, owned
        names or None, {name: rank} or None): the split file is the listing; no recording and no annotation is read"""
        import os
        with open(os.path.join(root, split + '.txt')) as f:
            lines = [ln for ln in f.readlines() if NCALTECH_BACKGROUND not in ln]
        listed = []
        for ln in lines:
            data_path, label_path = ln.strip().split(' ')
            listed.append((label_path.split('/')[-2], data_path.split('/')[-1].split('.')[0], os.path.join(root, data_path),
                           os.path.join(root, label_path)))
        names = [f'{c}-{stem}' for c, stem, _, _ in listed]
        owned, ranks = _shard_plan(names, [os.path.getsize(r[2]) for r in listed] if shard is not None else (), shard, None)
        return listed, names, owned, ranks

    @classmethod
    def _source_files(cls, root, split, shard):
        """the files ``from_directory`` with these arguments would open: the split file, every annotation, the owned recordings"""
        import os
        listed, names, owned, _ = cls._listed(root, split, shard)
        return ([os.path.join(root, split + '.txt')] + [label for _, _, _, label in listed]
                + [path for n, (_, _, path, _) in zip(names, listed) if owned is None or n in owned])

    def frames(self, sample_idx, params, exp, canvas_hw=None):
        """model input [B, Tl, Tm, 2, Hc, Wc] fp32 of the samples ``sample_idx`` (int64 [B] on the device): the store operator that
        ``exp.aggregation`` / ``exp.measure`` select, as ``atis_to_frames`` selects its own, on the B recordings alone, then the cubic
        letterbox; ``params``: (nw, nh, dx, dy, flip) per sample; ``canvas_hw``: ``exp.input_size`` unless given.  Nothing is read back
        (graph-capturable).  Precondition: the store holds the records of every sample asked for (``owns``; the loaders check their
        indices on the host before they upload them) -- a sample that is not owned has no records here."""
        op = {'latest': ops.event_latest_surface_atis_store, 'timesurface': ops.event_timesurface_atis_store,
              'count': ops.event_histogram_atis_store}[_atis_kind(exp)]
        frames = op(self.records, self.file_offsets, self.index, sample_idx, self.Tl, exp.Tm, *self.sensor_hw, window=self.window,
                    max_file_records=self.max_file_records)
        return _letterboxed(frames, params, canvas_hw if canvas_hw is not None else exp.input_size, 'cubic')

    def targets(self, sample_idx, params, canvas_hw, max_labels=50, return_info=False):
        """[B, max_labels, 5] fp32 rows (cls, cx, cy, w, h), zero padded, of the samples ``sample_idx`` under the draws ``params``:
        ``_Store.targets`` without a permutation (one box per sample), one launch, nothing read back"""
        return super().targets(sample_idx, params, None, canvas_hw, max_labels, return_info)


def ncaltech_store_for(exp, split='train', device=None):
    """The store of an experiment with ``train_input = 'atis_store'``: ``NCaltechStore.from_directory`` over ``exp.data_dir`` when it holds
    ``<split>.txt``, seeded synthetic recordings otherwise (``exp.atis_store_recordings`` = (files, events per file), default (16, 20000);
    the sensor is N-Caltech101's, or the canvas where that is smaller).  ``exp.store_shard`` = ``'recordings'``: the store of this rank.
    Kept on the experiment: one store per (split, rank, world, store_shard)."""
    import os
    window = (exp.window * 1000, 0) if getattr(exp, 'window', None) is not None else None
    root = str(getattr(exp, 'data_dir', '') or '')

    def synthetic(device, shard):
        n_files, n_events = getattr(exp, 'atis_store_recordings', (16, 20_000))
        size = exp.input_size if split == 'train' else exp.test_size
        sensor = (min(180, size[0]), min(240, size[1]))
        n_classes = max(int(exp.num_classes), 1)
        recs = synth_ncaltech_recordings(n_files, n_events, sensor, n_classes=n_classes, seed=int(split != 'train'))
        return NCaltechStore(recs, exp.Tl, window, device, class_names=[f'class_{i:03d}' for i in range(n_classes)], sensor_hw=sensor, shard=shard)
    return _store_for(exp, '_atis_stores', split, device, lambda: root and os.path.isfile(os.path.join(root, split + '.txt')) and root,
                      lambda root, device, shard: NCaltechStore.from_directory(root, split, exp.Tl, window, device, shard=shard), synthetic,
                      snapshot=lambda root, shard: ('atis_store', NCaltechStore, dict(Tl=int(exp.Tl), window=window, sensor_hw=(180, 240),
                                                                                      class_names=NCaltechStore._listed_classes(root)),
                                                    root, NCaltechStore._source_files(root, split, shard)))


class NCaltechStoreDataset(_StoreDataset):
    """``_StoreDataset`` over an ``NCaltechStore``: the class names are the store's"""

    def _class_names(self):
        return self.store.class_names


class NCaltechStoreLoader(_StoreLoader):
    """Training loader of N-Caltech101 from an ``NCaltechStore``: iterable of (frames [B, Tl, Tm, 2, Hc, Wc] fp32 on the GPU, targets
    [B, 50, 5] rows (cls, cx, cy, w, h), zero padded).  An epoch is a permutation of the samples; per sample the draws come in the reference's
    order (NCaltech.get_random_data, ncaltech.py:330-350): ``jitter_params(..., jitter=.1)`` and nothing else (``permutes`` is False:
    the reference's ``np.random.shuffle`` of the sample's single box consumes no random state, so none is drawn here).
    ``batches(epoch)`` returns the draws of an epoch, a function of (seed, epoch) alone; a step uploads them -- sample indices and
    params -- and everything else happens on the device (``store.frames``, ``store.targets``): no host read, no per-sample work.  ``store=None``: ``ncaltech_store_for(exp)``.  ``rank``, ``world`` and a sharded store: the rules of
    ``Gen1StoreLoader`` (rows ``rank::world`` of the global batch / a permutation of the owned samples from ``_shard_state``; the index
    check before the upload)."""
    jitter, permutes, what, Dataset = .1, False, 'recordings', NCaltechStoreDataset

    def check(self, exp):
        _atis_kind(exp)

    def make_store(self, exp):
        return ncaltech_store_for(exp)


class NCaltechStoreEvalLoader(_StoreEvalLoader):
    """Evaluation loader over an ``NCaltechStore``: iterable of the tuple ``Gen1StoreEvalLoader`` yields -- ``(frames [B, Tl, Tm, 2, H, W]
    fp32 on the GPU, labels [B][1, 5] rows (x, y, w, h, cls), (heights, widths), ids)``.  The frames go through the deterministic branch of
    get_random_data (``letterbox_params`` of the sensor on ``exp.test_size``, the cubic resize: N-Caltech101 resizes in evaluation too); the
    labels are the raw float32 rows of the store (``NCaltechStore.raw_labels``), prepared on the host once; the sizes are the sensor's and
    the ids index ``sample_names``.  ``indices`` are this rank's samples; the last batch may be short.  The index check and ``min_batches``
    are ``Gen1StoreEvalLoader``'s."""
    Dataset = NCaltechStoreDataset
