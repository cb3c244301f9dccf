"""Synthetic event streams and their GPU-side preprocessing (no real datasets in scope).

Stream definition = BASELINE.md section 2 / SURVEY.md 8d: per sample ``n_events`` events over a 200 ms window
on the 240x304 Gen1 sensor, ``t`` sorted uniform, ``x``,``y`` uniform, ``p`` Bernoulli(0.5), numpy default_rng.
Raw events (9 B/event) are what crosses PCIe; binning (K1) and canvas padding run on the GPU.
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


def events_to_frames(ev_dev, Tm, sensor_hw, canvas_hw, aggregation='micro_sum', tau=50e3):
    """Device events -> model input [B, Tl=1, Tm, 2, Hc, Wc] fp32 via the HIP histogram (K1).  ``aggregation='timesurface'``: Gen1's
    exponential time surfaces instead (``ops.event_time_surface`` with ``tau`` in us, gen1.py:362-369), placed like the counts: scale 1,
    top left, zero padding (``ops.frames_letterbox`` with ``unscaled_params``).  Any other value raises ValueError."""
    H, W = sensor_hw
    if check_aggregation(aggregation) == 'timesurface':
        surf = ops.event_time_surface(ev_dev['t'], ev_dev['x'], ev_dev['y'], ev_dev['p'], ev_dev['offsets'], Tm, H, W, tau=tau)
        return ops.frames_letterbox(surf, unscaled_params(surf.shape[0], sensor_hw, surf.device), canvas_hw[0], canvas_hw[1]).unsqueeze(1)
    frames = ops.event_frames(ev_dev['t'], ev_dev['x'], ev_dev['y'], ev_dev['p'], ev_dev['offsets'], Tm, H, W, canvas_hw[0], canvas_hw[1])
    return frames.unsqueeze(1)


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
        frames = ops.event_latest_surface_atis(records_dev, offsets_dev, Tl, Tm, H, W, window=window, tau=surface_tau)
        return ops.frames_letterbox(frames, params_on(params, frames.device), Hc, Wc, interp=interp)
    measure = 'count' if measure is None else measure
    if measure not in ATIS_MEASURES:
        raise ValueError(f"measure {measure!r}: the N-Caltech101 front end has {' and '.join(repr(m) for m in ATIS_MEASURES)}")
    if measure == 'timesurface':
        frames = ops.event_timesurface_atis(records_dev, offsets_dev, Tl, Tm, H, W, window=window, tau=tau)
        return ops.frames_letterbox(frames, params_on(params, frames.device), Hc, Wc, interp=interp)
    counts = ops.event_histogram_atis(records_dev, offsets_dev, Tl, Tm, H, W, window=window)
    return ops.counts_letterbox(counts, params_on(params, counts.device), Hc, Wc, interp=interp)


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
    if check_aggregation(aggregation) == 'timesurface':
        surf = ops.event_time_surface(ev_dev['t'], ev_dev['x'], ev_dev['y'], ev_dev['p'], ev_dev['offsets'], Tm, H, W, tau=tau)
        return ops.frames_letterbox(surf, params_on(params, surf.device), canvas_hw[0], canvas_hw[1]).unsqueeze(1)
    counts = ops.event_histogram(ev_dev['t'], ev_dev['x'], ev_dev['y'], ev_dev['p'], ev_dev['offsets'], Tm, H, W)
    return ops.counts_letterbox(counts, params_on(params, counts.device), canvas_hw[0], canvas_hw[1]).unsqueeze(1)


def dat_ranges_to_frames(records, ranges, Tm, sensor_hw, canvas_hw, params, aggregation='micro_sum', tau=50e3):
    """The Gen1 chain from record ranges: the .dat image ``records`` in HBM and the ranges int64 [B, 2] of ``ops.event_window_search`` ->
    model input [B, 1, Tm, 2, Hc, Wc] fp32, nothing read back in between (graph-capturable).  ``'micro_sum'``:
    ``ops.event_histogram_dat_ranges`` then ``ops.counts_letterbox``; ``'timesurface'``: ``ops.event_latest_surface_dat_ranges`` with ``tau``
    (us; GEN1Dataset.agrregate, gen1.py:362-369) then ``ops.frames_letterbox``, both with the linear resize; any other value raises
    ValueError.  ``params``: per-sample (nw, nh, dx, dy, flip) rows, a device int32 tensor or anything numpy reads."""
    H, W = sensor_hw
    if check_aggregation(aggregation) == 'timesurface':
        surf = ops.event_latest_surface_dat_ranges(records, ranges, Tm, H, W, tau=tau)
        return ops.frames_letterbox(surf, params_on(params, surf.device), canvas_hw[0], canvas_hw[1]).unsqueeze(1)
    counts = ops.event_histogram_dat_ranges(records, ranges, Tm, H, W)
    return ops.counts_letterbox(counts, params_on(params, counts.device), canvas_hw[0], canvas_hw[1]).unsqueeze(1)
