"""K1 and the other event representations: raw events / .dat records / stacked histograms -> count frames, voxel grids, time surfaces,
letterbox resize (reference: yolox/data/datasets/gen1.py:313-360, 433-521, psee_loader.py, event_reps.py, rvt_gen4.py:109-125).

Part of the operator layer of ``eas_snn_amd.ops`` (split by kernel family; ``ops`` re-exports everything here, so ``ops.<name>`` keeps working)."""
import ctypes as C

import torch

from . import _lib
from ._lib import check, ptr, stream
from .ops_core import _call, _dev, _f32c, _timer_add, _timer_mark


# ------------------------------------------------------------------------------------------------ K1
def event_histogram(t, x, y, p, sample_offsets, Tm, H, W, return_oob=False):
    """Per-sample micro-slice count frames: int32 [B, Tm, 2, H, W] (bit-exact 'micro_sum')."""
    _dev(t, x, y, p, sample_offsets)
    assert t.dtype == torch.uint32 or t.dtype == torch.int32, 't must be 32-bit timestamps'
    assert x.dtype in (torch.uint16, torch.int16) and y.dtype in (torch.uint16, torch.int16) and p.dtype in (torch.uint8, torch.int8)
    assert sample_offsets.dtype == torch.int64
    B = sample_offsets.numel() - 1
    out = torch.empty((B, Tm, 2, H, W), dtype=torch.int32, device=t.device)
    oob = torch.empty(1, dtype=torch.int32, device=t.device) if return_oob else None
    _call('eas_event_histogram', 9 * t.numel() + 4 * out.numel(), _lib.lib().eas_event_histogram, ptr(t), ptr(x), ptr(y), ptr(p),
          t.numel(), ptr(sample_offsets), B, Tm, H, W, ptr(out), ptr(oob), stream())
    return (out, oob) if return_oob else out


def event_histogram_dat(records, sample_offsets, Tm, H, W, return_oob=False):
    """Count frames int32 [B, Tm, 2, H, W] straight from .dat records: ``records`` is the raw byte image of the events
    (uint8 [8*nev], or any 8-byte-record view) already on the device; decode + binning happen in one kernel."""
    _dev(records, sample_offsets)
    assert sample_offsets.dtype == torch.int64
    rec = records.contiguous().view(torch.uint8)
    assert rec.numel() % 8 == 0, '.dat event records are 8 bytes'
    nev = rec.numel() // 8
    B = sample_offsets.numel() - 1
    out = torch.empty((B, Tm, 2, H, W), dtype=torch.int32, device=rec.device)
    oob = torch.empty(1, dtype=torch.int32, device=rec.device) if return_oob else None
    _call('eas_event_histogram_dat', 8 * nev + 4 * out.numel(), _lib.lib().eas_event_histogram_dat, ptr(rec), nev, ptr(sample_offsets), B, Tm,
          H, W, ptr(out), ptr(oob), stream())
    return (out, oob) if return_oob else out


def event_window_search(records, label_t, window, num_slice, file_offsets=None, file_id=None):
    """Record ranges int64 [B, 2] of the events GEN1Dataset.search_events returns for every label (gen1.py:217-232), found on the
    device.  records: the record area(s) of .dat recording(s) already in HBM (uint8 [8*nev] or any 8-byte-record view);
    label_t int64 [B] label timestamps (us); window = (lo, hi) us relative to the label; file_offsets int64 [F+1] (record index of
    every recording's first event; default: one recording) and file_id int32 [B]."""
    _dev(records, label_t, file_offsets, file_id)
    rec = records.contiguous().view(torch.uint8)
    assert rec.numel() % 8 == 0 and label_t.dtype == torch.int64
    nev = rec.numel() // 8
    if file_offsets is None:
        file_offsets = torch.tensor([0, nev], dtype=torch.int64, device=rec.device)
    assert file_offsets.dtype == torch.int64 and (file_id is None or file_id.dtype == torch.int32)
    B = label_t.numel()
    ranges = torch.empty((B, 2), dtype=torch.int64, device=rec.device)
    check(_lib.lib().eas_event_window_search(ptr(rec), ptr(file_offsets.contiguous()), file_offsets.numel() - 1,
                                             ptr(file_id.contiguous() if file_id is not None else None), ptr(label_t.contiguous()), B,
                                             int(window[0]), int(window[1]), int(num_slice), ptr(ranges), stream()), 'eas_event_window_search')
    return ranges


def record_ranges_union(ranges):
    """The union of the record ranges int64 [M, 2] (``event_window_search``; unsorted, overlapping, nested, duplicated, touching or empty
    with a == e) and where every range lies in it: ``segments`` int64 [S, 2] sorted, disjoint, non-empty (touching ranges merge),
    ``seg_dst`` int64 [S + 1] = the prefix of their lengths from 0, ``mapped`` int64 [M, 2] = every range's position in the segments laid back
    to back, of the range's own length (an empty range: (0, 0)).  Build-time plumbing on torch's sort and scans; S is read back once."""
    _dev(ranges)
    assert ranges.dtype == torch.int64 and ranges.dim() == 2 and ranges.shape[1] == 2
    a, e = ranges[:, 0], ranges[:, 1]
    full = e > a
    order = torch.argsort(torch.where(full, a, torch.iinfo(torch.int64).max))          # the empty ranges go last
    n = int(full.sum())
    sa, se = a[order[:n]], e[order[:n]]
    if n == 0:
        return ranges.new_zeros((0, 2)), ranges.new_zeros(1), torch.zeros_like(ranges)
    reach = torch.cummax(se, 0).values                                                  # how far the ranges in front of and at i reach
    first = torch.ones(n, dtype=torch.bool, device=ranges.device)
    first[1:] = sa[1:] > reach[:-1]                                                     # a gap in front: a segment begins (touching: none)
    starts = torch.nonzero(first).reshape(-1)
    seg_a = sa[starts]
    seg_e = reach[torch.cat([starts[1:], starts.new_tensor([n])]) - 1]
    seg_dst = torch.cat([seg_a.new_zeros(1), torch.cumsum(seg_e - seg_a, 0)])
    j = torch.searchsorted(seg_a, a.contiguous(), right=True).clamp_(min=1) - 1       # the segment that begins at or in front of a
    lo = torch.where(full, seg_dst[j] + (a - seg_a[j]), torch.zeros_like(a))
    return torch.stack([seg_a, seg_e], 1), seg_dst, torch.stack([lo, lo + (e - a).clamp(min=0)], 1)


def records_gather(src, segments, seg_dst, dst, dst_offset=0):
    """``dst[dst_offset + seg_dst[s] + i] = src[segments[s, 0] + i]`` for every record i of every segment s (``eas_records_gather``): the
    segments int64 [S, 2] of ``record_ranges_union`` copied back to back into ``dst`` from record ``dst_offset`` on.  ``src``, ``dst``: uint8
    images of 8-byte records (or any 8-byte-record view) on the device, not overlapping.  The segments are checked against both buffers on the
    host (one read per call: build time); returns the number of records copied."""
    _dev(src, segments, seg_dst, dst)
    s8, d8 = src.view(torch.uint8), dst.view(torch.uint8)
    assert src.is_contiguous() and dst.is_contiguous() and s8.numel() % 8 == 0 and d8.numel() % 8 == 0, 'records are 8 bytes'
    assert segments.dtype == torch.int64 and segments.dim() == 2 and segments.shape[1] == 2 and seg_dst.dtype == torch.int64
    S = segments.shape[0]
    assert seg_dst.shape == (S + 1,) and int(dst_offset) >= 0
    if S == 0:
        return 0
    length = segments[:, 1] - segments[:, 0]
    ok = (length >= 0).all() & (length == seg_dst[1:] - seg_dst[:-1]).all() & (segments[:, 0] >= 0).all() & (segments[:, 1] <= s8.numel() // 8).all()
    ok, first, last = torch.stack([ok.to(torch.int64), seg_dst[0], seg_dst[-1]]).tolist()
    if not ok or first < 0 or int(dst_offset) + last > d8.numel() // 8:
        raise ValueError(f'records_gather: the segments do not fit (source {s8.numel() // 8} records, destination {d8.numel() // 8} records, '
                         f'offset {int(dst_offset)}, span {first}..{last})')
    seg_src, seg_pos = segments[:, 0].contiguous(), seg_dst + int(dst_offset)       # two tables of their own, alive until the call is enqueued
    _call('eas_records_gather', 16 * (last - first), _lib.lib().eas_records_gather, ptr(s8), ptr(seg_src), ptr(seg_pos), S, last - first,
          ptr(d8), stream())
    return last - first


_DIGEST_GOLDEN, _DIGEST_M1, _DIGEST_M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_DIGEST_HOST_WORDS = 1 << 20         # words per step of the host evaluation (8 MiB of the buffer, a few arrays of that size beside it)


def _bytes_digest_numpy(raw):
    """(sum, xor) of ``eas_bytes_digest``'s definition (include/eas_hip.h) on the uint8 numpy array ``raw``, with numpy: what a store kept
    on the host is digested by.  The same function as the kernel's, word for word; evaluated ``_DIGEST_HOST_WORDS`` words at a time."""
    import numpy as np
    raw = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    n = (raw.size + 7) // 8
    s, x = np.uint64(0), np.uint64(0)
    for a in range(0, n, _DIGEST_HOST_WORDS):
        e = min(a + _DIGEST_HOST_WORDS, n)
        part = raw[8 * a:8 * e]
        if part.size != 8 * (e - a):                        # the last word: its missing bytes are zero
            part = np.concatenate([part, np.zeros(8 * (e - a) - part.size, np.uint8)])
        z = part.view('<u8').astype(np.uint64) + np.arange(a + 1, e + 1, dtype=np.uint64) * np.uint64(_DIGEST_GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_DIGEST_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_DIGEST_M2)
        z = z ^ (z >> np.uint64(31))
        s, x = s + np.add.reduce(z, dtype=np.uint64), x ^ np.bitwise_xor.reduce(z)
    return int(s), int(x)


def bytes_digest(t):
    """``torch.uint64`` [2] on ``t.device``: the 128-bit digest (sum, xor) of the bytes of the contiguous tensor ``t``
    (``eas_bytes_digest``, include/eas_hip.h: a corruption check, not a cryptographic hash; the byte length is not part of it).  One reading
    pass on the device, nothing read back (graph-capturable); a view that does not start on 16 bytes is cloned first.  A CPU tensor is
    digested by the same definition with numpy -- the one operator that takes one: the stores that are built on the host need it."""
    assert t.is_contiguous(), 'bytes_digest reads the bytes of a contiguous tensor'
    flat = t.reshape(-1).view(torch.uint8)
    if not t.is_cuda:
        import numpy as np
        with np.errstate(over='ignore'):
            words = _bytes_digest_numpy(flat.numpy())
        return torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64)).view(torch.uint64)
    if flat.data_ptr() % 16:
        flat = flat.clone()
    out = torch.empty(2, dtype=torch.uint64, device=t.device)
    _call('eas_bytes_digest', flat.numel(), _lib.lib().eas_bytes_digest, ptr(flat) if flat.numel() else None, flat.numel(), ptr(out), stream())
    return out


def bytes_digest_host(t):
    """``bytes_digest(t)`` as two Python ints (sum, xor): the one place that reads the two words back"""
    words = bytes_digest(t).view(torch.int64).cpu().numpy().view('<u8')
    return int(words[0]), int(words[1])


def _dat_ranges_frames(timer, entry, dtype, out_bytes, records, ranges, ns, H, W, tau, return_oob):
    """the two .dat-range wrappers: checks, allocations, the call (``tau``: a tuple, empty for the counts) and the return tuple"""
    _dev(records, ranges)
    rec = records.contiguous().view(torch.uint8)
    assert rec.numel() % 8 == 0, '.dat event records are 8 bytes'
    assert ranges.dtype == torch.int64 and ranges.dim() == 2 and ranges.shape[1] == 2
    B = ranges.shape[0]
    out = torch.empty((B, ns, 2, H, W), dtype=dtype, device=rec.device)
    oob = torch.empty(1, dtype=torch.int32, device=rec.device) if return_oob else None
    _call(timer, 8 * (rec.numel() // 8) + out_bytes * out.numel(), getattr(_lib.lib(), entry), ptr(rec), ptr(ranges.contiguous()), B, ns, H, W,
          *tau, ptr(out), ptr(oob), stream())
    return (out, oob) if return_oob else out


def event_histogram_dat_ranges(records, ranges, Tm, H, W, return_oob=False):
    """Count frames int32 [B, Tm, 2, H, W] of the record ranges [B, 2] (``event_window_search``) of a .dat image in HBM: label
    timestamps in, frames out, nothing read back to the host in between."""
    return _dat_ranges_frames('eas_event_histogram_dat', 'eas_event_histogram_dat_ranges', torch.int32, 4, records, ranges, Tm, H, W, (), return_oob)


def _atis_frames(entry, dtype, workspace_query, out_bytes, records, sample_offsets, Tl, Tm, H, W, window, tau, return_oob, return_flags):
    """the three ATIS wrappers: checks, the window rule, allocations, the call (``tau``: a tuple, empty for the counts) and the return tuple.
    bytes: the records twice + ``out_bytes`` per element of the frames"""
    _dev(records, sample_offsets)
    assert records.dtype == torch.uint8 and sample_offsets.dtype == torch.int64
    rec = records if records.is_contiguous() else records.contiguous()
    assert rec.numel() % 5 == 0, 'ATIS records are 5 bytes'
    nrec = rec.numel() // 5
    B = sample_offsets.numel() - 1
    lo, hi = (0, 0) if window is None or window[0] >= 0 else (int(window[0]), int(window[1]))
    out = torch.empty((B, Tl, Tm, 2, H, W), dtype=dtype, device=rec.device)
    oob = torch.empty(B, dtype=torch.int32, device=rec.device) if return_oob else None
    flags = torch.empty(B, dtype=torch.int32, device=rec.device) if return_flags else None
    ws = torch.empty(getattr(_lib.lib(), workspace_query)(nrec, B, Tl), dtype=torch.uint8, device=rec.device)
    _call(entry, 10 * nrec + out_bytes * out.numel(), getattr(_lib.lib(), entry), ptr(rec), nrec, ptr(sample_offsets.contiguous()), B, lo, hi,
          Tl, Tm, H, W, *tau, ptr(out), ptr(oob), ptr(flags), ptr(ws), stream())
    res = (out,) + ((oob,) if return_oob else ()) + ((flags,) if return_flags else ())
    return res if len(res) > 1 else out


def event_histogram_atis(records, sample_offsets, Tl, Tm, H, W, window=None, return_oob=False, return_flags=False):
    """Count frames int32 [B, Tl, Tm, 2, H, W] straight from raw ATIS recordings (N-Caltech101 ``.bin``, 5 bytes per record) in HBM:
    decode with overflow records, ``window`` (lo, hi) us relative to the last event (None or lo >= 0: no window), the reference's macro /
    micro slicing and the count histogram on the device (NCaltech.read_ATIS / generate_slices / agrregate 'micro_sum').  ``records``: any
    uint8 view, at any alignment; ``sample_offsets`` int64 [B+1] record indices.  Optional returns: out-of-sensor events per recording
    (int32 [B]) and flags (int32 [B]; bit 0 event times decrease, bit 1 no event remains / a macro slice is empty)."""
    return _atis_frames('eas_event_histogram_atis', torch.int32, 'eas_event_histogram_atis_workspace_bytes', 4, records, sample_offsets, Tl, Tm, H, W,
                        window, (), return_oob, return_flags)


def event_timesurface_atis(records, sample_offsets, Tl, Tm, H, W, window=None, tau=500e3, return_oob=False, return_flags=False):
    """``event_histogram_atis`` with the reference's measure 'timesurface': float64 frames [B, Tl, Tm, 2, H, W] in which every event adds
    ``1 - tanh((t_target - t) / tau)`` instead of 1, ``t_target`` the time of the last event of its macro slice, ``tau`` in us
    (NCaltech.get_measure_func, ncaltech.py:218-225; event_reps.py:13-19).  Same decode, window, slicing and optional returns; flags bit 2:
    a macro slice spans more records than one bin can hold at weight 1 (``eas_event_timesurface_atis_capacity()``).  Bit-identical from run
    to run (64-bit integer sums of the weights in units of 2^-48)."""
    # bytes: the 64-bit bins written, then read and written once more by the finishing pass
    return _atis_frames('eas_event_timesurface_atis', torch.float64, 'eas_event_timesurface_atis_workspace_bytes', 24, records, sample_offsets, Tl, Tm,
                        H, W, window, (float(tau),), return_oob, return_flags)


def event_latest_surface_atis(records, sample_offsets, Tl, Tm, H, W, window=None, tau=10e3, return_oob=False, return_flags=False):
    """The reference's ``aggregation timesurface`` of raw ATIS recordings: float64 [B, Tl, Tm, 2, H, W], frame ``q`` of a macro slice =
    ``exp(-((q + 1) * w + f - latest) / tau)`` on every pixel, ``latest`` the time of the pixel's last event in micro slices 0 .. q of the
    macro slice (0 where none fell: a surface is > 0 everywhere), ``f`` / ``w`` the macro slice's first time and micro window, ``tau`` in us
    (NCaltech.agrregate 'timesurface', ncaltech.py:255-257; to_timesurface_numpy, event_reps.py:141-160).  Decode, window, slicing and the
    optional returns are ``event_histogram_atis``'s; flags bit 3 (value 8): a macro slice holds events and has micro window 0 (the reference
    raises; its frames are zero).  Not ``event_timesurface_atis``, which is the *measure* of that name.  Bit-identical from run to run."""
    # bytes: the 64-bit bins zeroed, then read and written once by the finishing pass
    return _atis_frames('eas_event_latest_surface_atis', torch.float64, 'eas_event_histogram_atis_workspace_bytes', 24, records, sample_offsets, Tl, Tm,
                        H, W, window, (float(tau),), return_oob, return_flags)


def atis_store_index(records):
    """The overflow index of a buffer of ATIS recordings resident in HBM: uint32 [chunks + 1] (as an int32 tensor), entry c = overflow
    records in front of record 256 * c, the last entry all of them.  Two launches over the buffer, once per store; the ``*_atis_store``
    operators take it with the ``records`` it was made from (the same view: chunks are counted from its first byte)."""
    _dev(records)
    assert records.dtype == torch.uint8 and records.is_contiguous() and records.numel() % 5 == 0, 'ATIS records are 5 bytes'
    nrec = records.numel() // 5
    index = torch.empty(_lib.lib().eas_atis_store_index_bytes(nrec) // 4, dtype=torch.int32, device=records.device)
    _call('eas_atis_store_index', 5 * nrec + 8 * index.numel(), _lib.lib().eas_atis_store_index, ptr(records), nrec, ptr(index), stream())
    return index


def _atis_store_frames(entry, dtype, workspace_query, out_bytes, records, file_offsets, index, sample_file, Tl, Tm, H, W, window, tau, return_oob,
                       return_flags, max_file_records):
    """the three store wrappers: ``_atis_frames`` for recordings picked out of a resident store.  bytes: at most ``max_file_records`` records
    per sample, once, + ``out_bytes`` per element of the frames -- not the store"""
    _dev(records, file_offsets, index, sample_file)
    assert records.dtype == torch.uint8 and records.is_contiguous() and records.numel() % 5 == 0, 'ATIS records are 5 bytes'
    assert file_offsets.dtype == torch.int64 and file_offsets.dim() == 1 and file_offsets.numel() >= 1 and file_offsets.is_contiguous()
    assert sample_file.dtype == torch.int64 and sample_file.dim() == 1
    nrec, F, B = records.numel() // 5, file_offsets.numel() - 1, sample_file.numel()
    assert index.dtype == torch.int32 and index.is_contiguous() and index.numel() == _lib.lib().eas_atis_store_index_bytes(nrec) // 4, \
        'the index is not atis_store_index(records)'
    max_file_records = nrec if max_file_records is None else int(max_file_records)
    lo, hi = (0, 0) if window is None or window[0] >= 0 else (int(window[0]), int(window[1]))
    out = torch.empty((B, Tl, Tm, 2, H, W), dtype=dtype, device=records.device)
    oob = torch.empty(B, dtype=torch.int32, device=records.device) if return_oob else None
    flags = torch.empty(B, dtype=torch.int32, device=records.device) if return_flags else None
    ws = torch.empty(getattr(_lib.lib(), workspace_query)(B, Tl), dtype=torch.uint8, device=records.device)
    _call(entry, 5 * max_file_records * B + out_bytes * out.numel(), getattr(_lib.lib(), entry), ptr(records), nrec, ptr(file_offsets), F,
          ptr(sample_file.contiguous()), B, ptr(index), max_file_records, lo, hi, Tl, Tm, H, W, *tau, ptr(out), ptr(oob), ptr(flags), ptr(ws), stream())
    res = (out,) + ((oob,) if return_oob else ()) + ((flags,) if return_flags else ())
    return res if len(res) > 1 else out


def event_histogram_atis_store(records, file_offsets, index, sample_file, Tl, Tm, H, W, window=None, return_oob=False, return_flags=False,
                               max_file_records=None):
    """``event_histogram_atis`` of recordings picked out of a store resident in HBM: ``records`` uint8 (every recording back to back),
    ``file_offsets`` int64 [F + 1] record indices, ``index`` = ``atis_store_index(records)``, ``sample_file`` int64 [B] (recording b of the
    batch is file ``sample_file[b]``; an index may repeat) -> int32 [B, Tl, Tm, 2, H, W], bit for bit what the packed operator gives on those
    recordings.  The work is the batch's: nothing outside the B recordings is counted or scanned.  ``max_file_records``: the store's longest
    recording (None: the whole buffer); it sizes the grid only.  An entry outside [0, F) gives zero frames and flags bit 4 (value 16) besides
    bit 1.  Nothing is read back (graph-capturable)."""
    return _atis_store_frames('eas_event_histogram_atis_store', torch.int32, 'eas_atis_store_workspace_bytes', 4, records, file_offsets, index,
                              sample_file, Tl, Tm, H, W, window, (), return_oob, return_flags, max_file_records)


def event_timesurface_atis_store(records, file_offsets, index, sample_file, Tl, Tm, H, W, window=None, tau=500e3, return_oob=False,
                                 return_flags=False, max_file_records=None):
    """``event_timesurface_atis`` (measure 'timesurface') on a store: the arguments of ``event_histogram_atis_store``, float64 frames"""
    return _atis_store_frames('eas_event_timesurface_atis_store', torch.float64, 'eas_atis_store_timesurface_workspace_bytes', 24, records,
                              file_offsets, index, sample_file, Tl, Tm, H, W, window, (float(tau),), return_oob, return_flags, max_file_records)


def event_latest_surface_atis_store(records, file_offsets, index, sample_file, Tl, Tm, H, W, window=None, tau=10e3, return_oob=False,
                                    return_flags=False, max_file_records=None):
    """``event_latest_surface_atis`` (aggregation 'timesurface') on a store: the arguments of ``event_histogram_atis_store``, float64 frames"""
    return _atis_store_frames('eas_event_latest_surface_atis_store', torch.float64, 'eas_atis_store_workspace_bytes', 24, records, file_offsets,
                              index, sample_file, Tl, Tm, H, W, window, (float(tau),), return_oob, return_flags, max_file_records)


def event_latest_surface_dat_ranges(records, ranges, num_slices, H, W, tau=50e3, return_oob=False):
    """``event_time_surface`` (Gen1's ``aggregation timesurface``) of the record ranges [B, 2] (``event_window_search``) of a .dat image in
    HBM: float64 [B, num_slices, 2, H, W], bit-identical to ``event_time_surface`` on the decoded arrays of the same samples; an empty range
    or a window of zero length gives zero frames.  Label timestamps in, surfaces out, nothing read back to the host in between.  Optional
    return: the events outside the sensor that were dropped (int32 [1])."""
    return _dat_ranges_frames('eas_event_latest_surface_dat_ranges', 'eas_event_latest_surface_dat_ranges', torch.float64, 24, records, ranges,
                              num_slices, H, W, (float(tau),), return_oob)


def event_frames(t, x, y, p, sample_offsets, Tm, H, W, Hc, Wc):
    """raw events -> fp32 count frames on the zero-padded model canvas [B, Tm, 2, Hc, Wc] in one call (K1 + canvas)."""
    _dev(t, x, y, p, sample_offsets)
    B = sample_offsets.numel() - 1
    out = torch.empty((B, Tm, 2, Hc, Wc), dtype=torch.float32, device=t.device)
    scratch = torch.empty((B, Tm, 2, H, W), dtype=torch.int32, device=t.device)
    _call('eas_event_histogram', 9 * t.numel() + 4 * out.numel(), _lib.lib().eas_event_frames, ptr(t), ptr(x), ptr(y), ptr(p), t.numel(),
          ptr(sample_offsets), B, Tm, H, W, Hc, Wc, ptr(out), ptr(scratch), None, stream())
    return out


def stacked_hist_event_sum(hist, Hc, Wc, nbins=10, n_valid=None):
    """RVT stacked histogram u8 [B, Tm, 2*nbins, H, W] -> fp32 model input [B, 1, Tm, 2, Hc, Wc]: sum over the time bins of each
    polarity, zero padded to the canvas (RVTGEN4Dataset.generate_slices 'event_sum' + validation letterbox, rvt_gen4.py:109-125,
    516-533).  n_valid int32 [B]: samples that supply only their first n_valid[b] slices (zero slices in front)."""
    _dev(hist, n_valid)
    assert hist.dtype == torch.uint8 and hist.dim() == 5 and hist.shape[2] == 2 * nbins
    hist = hist.contiguous()
    B, Tm, _, H, W = hist.shape
    if n_valid is not None:
        assert n_valid.dtype == torch.int32 and n_valid.shape == (B,)
        n_valid = n_valid.contiguous()
    out = torch.empty((B, 1, Tm, 2, Hc, Wc), dtype=torch.float32, device=hist.device)
    _call('eas_stacked_hist_event_sum', hist.numel() + 4 * out.numel(), _lib.lib().eas_stacked_hist_event_sum, ptr(hist), ptr(n_valid), B, Tm,
          int(nbins), H, W, Hc, Wc, ptr(out), stream())
    return out


def stacked_hist_frames(store, first, Tm, Hc, Wc, nbins=10, lo=None, params=None, return_flags=False):
    """The 1 Mpx training input from indices: ``store`` u8 [R, 2*nbins, H, W] (the representations of one or more recordings back to back,
    resident in HBM), ``first`` int64 [B] (index of the representation that feeds output slice 0: ``data.rvt_first_index``) -> fp32 model
    input [B, 1, Tm, 2, Hc, Wc]: bin sums of slices first[b] .. first[b] + Tm - 1, resized / pasted / flipped by ``params`` int32 [B, 5] =
    (nw, nh, dx, dy, flip) with cv2 INTER_LINEAR semantics (None: (W, H, 0, 0, 0), the validation letterbox at scale 1), bit-identical to
    ``counts_letterbox`` of the int32 bin sums (RVTGEN4Dataset.__getitem__, rvt_gen4.py:190-235).  ``lo`` int64 [B] (None: 0): first
    representation of each sample's recording; slices below it are zero (a young sequence).  A slice at or behind R is zero too and sets
    bit 0 of the sample's flag (``return_flags``: also int32 [B])."""
    _dev(store, first, lo, params)
    assert store.dtype == torch.uint8 and store.dim() == 4 and store.shape[1] == 2 * nbins
    assert first.dtype == torch.int64 and first.dim() == 1
    store, first = store.contiguous(), first.contiguous()
    R, _, H, W = store.shape
    B = first.numel()
    if lo is not None:
        assert lo.dtype == torch.int64 and lo.shape == (B,)
        lo = lo.contiguous()
    if params is not None:
        assert params.dtype == torch.int32 and params.shape == (B, 5)
        params = params.contiguous()
    out = torch.empty((B, 1, Tm, 2, Hc, Wc), dtype=torch.float32, device=store.device)
    flags = torch.empty(B, dtype=torch.int32, device=store.device) if return_flags else None
    # bytes: every source row at most once per (sample, slice) + the frames (a downscale reads fewer rows)
    _call('eas_stacked_hist_frames', B * Tm * 2 * nbins * H * W + 4 * out.numel(), _lib.lib().eas_stacked_hist_frames, ptr(store), R, ptr(first),
          ptr(lo), ptr(params), B, int(Tm), int(nbins), H, W, Hc, Wc, ptr(out), ptr(flags), stream())
    return (out, flags) if return_flags else out


def stacked_hist_bin_sums(hist, nbins=10, out=None):
    """The builder of a summed store: ``hist`` u8 [n, 2*nbins, H, W] (channel = polarity * nbins + bin) -> ``torch.uint16`` [n, 2, H, W], the sum
    over the time bins of each polarity (exact: at most 255 * nbins <= 65025).  ``out``: a contiguous view into a store allocated once
    (``store[a:a + n]``) that the call fills and returns -- a recording is summed chunk by chunk as it is uploaded and its u8 form never
    exists whole on the device.  n = 0 is no launch.  Nothing is read back."""
    _dev(hist, out)
    assert hist.dtype == torch.uint8 and hist.dim() == 4 and hist.shape[1] == 2 * nbins
    hist = hist.contiguous()
    n, _, H, W = hist.shape
    if out is None:
        out = torch.empty((n, 2, H, W), dtype=torch.uint16, device=hist.device)
    assert out.dtype == torch.uint16 and out.shape == (n, 2, H, W) and out.is_contiguous() and out.device == hist.device
    if n == 0:                               # (an empty tensor has no address to hand to the entry)
        return out
    _call('eas_stacked_hist_bin_sums', hist.numel() + 2 * out.numel(), _lib.lib().eas_stacked_hist_bin_sums, ptr(hist), n, int(nbins), H, W,
          ptr(out), stream())
    return out


def count_store_frames(sums, first, Tm, Hc, Wc, lo=None, params=None, return_flags=False):
    """``stacked_hist_frames`` on a summed store: ``sums`` ``torch.uint16`` [R, 2, H, W] (``stacked_hist_bin_sums`` of the representations of one
    or more recordings back to back, resident in HBM) -> fp32 model input [B, 1, Tm, 2, Hc, Wc], bit-identical to ``stacked_hist_frames`` on
    the unsummed store with the same ``first``, ``lo``, ``params`` (their meaning, the clamping, the zero slices and the flag bit are that
    operator's).  Nothing is read back (graph-capturable)."""
    _dev(sums, first, lo, params)
    assert sums.dtype == torch.uint16 and sums.dim() == 4 and sums.shape[1] == 2
    assert first.dtype == torch.int64 and first.dim() == 1
    sums, first = sums.contiguous(), first.contiguous()
    R, _, H, W = sums.shape
    B = first.numel()
    if lo is not None:
        assert lo.dtype == torch.int64 and lo.shape == (B,)
        lo = lo.contiguous()
    if params is not None:
        assert params.dtype == torch.int32 and params.shape == (B, 5)
        params = params.contiguous()
    out = torch.empty((B, 1, Tm, 2, Hc, Wc), dtype=torch.float32, device=sums.device)
    flags = torch.empty(B, dtype=torch.int32, device=sums.device) if return_flags else None
    # bytes: every source row at most once per (sample, slice), two bytes per pixel, + the frames (a downscale reads fewer rows)
    _call('eas_count_store_frames', B * Tm * 2 * 2 * H * W + 4 * out.numel(), _lib.lib().eas_count_store_frames, ptr(sums), R, ptr(first), ptr(lo),
          ptr(params), B, int(Tm), H, W, Hc, Wc, ptr(out), ptr(flags), stream())
    return (out, flags) if return_flags else out


PACKED_MAX_W = 1024          # 64 groups of 16 pixels: one bit each in the two masks of a row


class PackedArenaFull(ValueError):
    """``count_rows_pack`` found the arena too small; ``units``: what the chunk takes (nothing was written to the arena)"""

    def __init__(self, msg, units):
        super().__init__(msg)
        self.units = units


def _packed_rows_args(sums, table, payload):
    """the shapes and types the three row operators share; returns (n, H, W)"""
    _dev(sums, table, payload)
    assert sums.dtype == torch.uint16 and sums.dim() == 4 and sums.shape[1] == 2 and sums.is_contiguous()
    n, _, H, W = sums.shape
    if W > PACKED_MAX_W:
        raise ValueError(f'packed rows hold at most 64 groups of 16 pixels: W = {W} > {PACKED_MAX_W}')
    assert table.dtype == torch.int64 and table.shape == (n, 2, H, 3) and table.is_contiguous() and table.device == sums.device
    assert payload.dtype == torch.uint8 and payload.dim() == 1 and payload.is_contiguous() and payload.device == sums.device
    return n, H, W


def count_rows_pack(sums, table_out, payload, unit_offset, dry_run=False):
    """Packs the bin sums ``sums`` ``torch.uint16`` [n, 2, H, W] (``stacked_hist_bin_sums``) into rows of 16-pixel groups -- a zero group stores
    nothing, a group whose maximum is at most 255 16 bytes, any other 32 (include/eas_hip.h states the format) -- behind unit ``unit_offset``
    (units of 16 bytes) of the arena ``payload`` (uint8 [capacity], 16-byte aligned), and fills ``table_out`` int64 [n, 2, H, 3] = (nz, wide,
    offset) -- a contiguous view into a table allocated once (``table[a:a + n]``).  Three steps: ``eas_count_rows_measure`` (masks and units
    of every row), an exclusive scan of the units on the device plus ``unit_offset``, ``eas_count_rows_pack``.  Returns the units used: the one
    value a call reads back.  An arena that cannot take them raises ``PackedArenaFull`` (a ValueError that names the bytes needed) before
    anything is written to it; ``dry_run``: measure and fill the table only, the arena is neither checked nor written.  W > 1024 raises
    ValueError."""
    n, H, W = _packed_rows_args(sums, table_out, payload)
    unit_offset = int(unit_offset)
    assert unit_offset >= 0
    if n == 0:
        return 0
    _call('eas_count_rows_measure', 2 * sums.numel() + 8 * table_out.numel(), _lib.lib().eas_count_rows_measure, ptr(sums), n, H, W, ptr(table_out),
          stream())
    third = table_out[..., 2]
    ends = torch.cumsum(third.reshape(-1), 0)
    units = int(ends[-1])                                      # (the read of a build step)
    third.copy_((ends - third.reshape(-1) + unit_offset).reshape(third.shape))
    if dry_run:
        return units
    if (unit_offset + units) * 16 > payload.numel():
        raise PackedArenaFull(f'the packed rows need {(unit_offset + units) * 16} bytes, the arena holds {payload.numel()}', units)
    _call('eas_count_rows_pack', 2 * sums.numel() + 8 * table_out.numel() + 16 * units, _lib.lib().eas_count_rows_pack, ptr(sums), n, H, W,
          ptr(table_out), ptr(payload), unit_offset, unit_offset + units, stream())
    return units


def count_rows_unpack(table, payload, W):
    """The inverse of ``count_rows_pack``: ``table`` int64 [n, 2, H, 3] (the rows of n representations, a contiguous view ``table[a:b]`` of a
    store's table; the offsets stay positions in the whole ``payload``) and ``payload`` uint8 [used bytes] -> ``torch.uint16`` [n, 2, H, W]."""
    _dev(table, payload)
    assert table.dtype == torch.int64 and table.dim() == 4 and table.shape[1] == 2 and table.shape[3] == 3 and table.is_contiguous()
    n, _, H, _ = table.shape
    sums = torch.empty((n, 2, H, int(W)), dtype=torch.uint16, device=table.device)
    _packed_rows_args(sums, table, payload)
    if n:
        _call('eas_count_rows_unpack', 2 * sums.numel() + 8 * table.numel() + payload.numel(), _lib.lib().eas_count_rows_unpack, ptr(table),
              ptr(payload), payload.numel() // 16, n, H, int(W), ptr(sums), stream())
    return sums


def packed_store_frames(table, payload, first, Tm, Hc, Wc, lo=None, params=None, return_flags=False, *, W):
    """``count_store_frames`` on a store in packed rows: ``table`` int64 [R, 2, H, 3] and ``payload`` uint8 [used bytes] (``count_rows_pack`` of
    the bin sums of one or more recordings back to back; ``W``, by keyword: the sensor's width, which the table does not carry) -> fp32 model input
    [B, 1, Tm, 2, Hc, Wc], bit-identical to ``count_store_frames`` on those sums with the same ``first``, ``lo``, ``params``.  Nothing is read
    back (graph-capturable)."""
    _dev(table, payload, first, lo, params)
    assert table.dtype == torch.int64 and table.dim() == 4 and table.shape[1] == 2 and table.shape[3] == 3
    assert payload.dtype == torch.uint8 and payload.dim() == 1
    assert first.dtype == torch.int64 and first.dim() == 1
    if W > PACKED_MAX_W:
        raise ValueError(f'packed rows hold at most 64 groups of 16 pixels: W = {W} > {PACKED_MAX_W}')
    table, payload, first = table.contiguous(), payload.contiguous(), first.contiguous()
    R, _, H, _ = table.shape
    B = first.numel()
    if lo is not None:
        assert lo.dtype == torch.int64 and lo.shape == (B,)
        lo = lo.contiguous()
    if params is not None:
        assert params.dtype == torch.int32 and params.shape == (B, 5)
        params = params.contiguous()
    out = torch.empty((B, 1, Tm, 2, Hc, Wc), dtype=torch.float32, device=table.device)
    flags = torch.empty(B, dtype=torch.int32, device=table.device) if return_flags else None
    # bytes: at most what the u16 store reads (every group wide) + the row words + the frames
    _call('eas_packed_store_frames', B * Tm * 2 * H * (2 * int(W) + 24) + 4 * out.numel(), _lib.lib().eas_packed_store_frames, ptr(table), ptr(payload),
          payload.numel() // 16, R, ptr(first), ptr(lo), ptr(params), B, int(Tm), H, int(W), Hc, Wc, ptr(out), ptr(flags), stream())
    return (out, flags) if return_flags else out


RECORDS_BLOCK, RECORDS_UNIT = 64, 256       # records per block of the packed records; bytes per payload unit (narrow block: 1, wide: 2)
RECORDS_FLAG_RANGE, RECORDS_FLAG_TABLE = 1, 2       # flag bits of the packed-range operators: a refused range / a table entry outside the payload


def records_widths(H, W):
    """(XB, YB, DB) of packed records on an ``H`` x ``W`` sensor: bits of W - 1 and of H - 1 (each at least 1) and what 31 bits leave for the
    time offset inside a block; ValueError where that is fewer than 8 bits or a side exceeds the record's 14-bit fields"""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f'a sensor of {H} x {W}')
    xb, yb = max((W - 1).bit_length(), 1), max((H - 1).bit_length(), 1)
    if 31 - xb - yb < 8 or H > 16384 or W > 16384:
        raise ValueError(f'packed records: a sensor of {H} x {W} takes {xb} + {yb} bits and leaves {31 - xb - yb} for the time (8 at least)')
    return xb, yb, 31 - xb - yb


def _packed_records_args(table, payload):
    """the shapes and types of a packed store; returns (blocks, units)"""
    _dev(table, payload)
    assert table.dtype == torch.int32 and table.dim() == 2 and table.shape[1] == 2 and table.is_contiguous()
    assert payload.dtype == torch.uint8 and payload.dim() == 1 and payload.is_contiguous() and payload.device == table.device
    return table.shape[0], payload.numel() // RECORDS_UNIT


def records_pack(records, table_out, payload, unit_offset, H, W, dry_run=False):
    """Packs the 8-byte records ``records`` (uint8 [8 * n] or any 8-byte-record view, on the device) in blocks of 64 -- a narrow block 256
    bytes, a wide block 512 (include/eas_hip.h states the format) -- behind unit ``unit_offset`` (units of 256 bytes) of the arena
    ``payload`` (uint8 [capacity], 16-byte aligned), and fills ``table_out`` int32 [ceil(n / 64), 2] = the bit patterns of (base time, unit |
    wide << 31) -- a contiguous view into a table allocated once.  Three steps: ``eas_records_pack_measure`` (base and units of every block),
    an exclusive scan of the units on the device plus ``unit_offset``, ``eas_records_pack``.  The records behind record n - 1 in the last
    block are copies of it.  Returns the units used: the one value a call reads back.  An arena that cannot take them raises
    ``PackedArenaFull`` (a ValueError that names the bytes needed) before anything is written to it; ``dry_run``: measure and fill the table
    only, the arena is neither checked nor written.  A sensor that leaves fewer than 8 bits for the time raises ValueError."""
    records_widths(H, W)
    _dev(records)
    rec = records.view(torch.uint8)
    assert records.is_contiguous() and rec.dim() == 1 and rec.numel() % 8 == 0, 'records are 8 bytes'
    n, unit_offset = rec.numel() // 8, int(unit_offset)
    nb = (n + RECORDS_BLOCK - 1) // RECORDS_BLOCK
    _packed_records_args(table_out, payload)
    assert table_out.shape[0] == nb and table_out.device == rec.device and unit_offset >= 0
    if n == 0:
        return 0
    _call('eas_records_pack_measure', 8 * n + 8 * nb, _lib.lib().eas_records_pack_measure, ptr(rec), n, int(H), int(W), ptr(table_out), stream())
    second = table_out[:, 1]
    ends = torch.cumsum(second, 0, dtype=torch.int64)
    units = int(ends[-1])                                      # (the read of a build step)
    if unit_offset + units > 1 << 31:
        raise ValueError(f'packed records: unit {unit_offset + units} is beyond the 2^31 units (512 GB) a table addresses')
    # the place, and the wide flag in bit 31: as int32, place - 2^31
    second.copy_(ends - second + unit_offset - (second == 2).to(torch.int64) * (1 << 31))
    if dry_run:
        return units
    if (unit_offset + units) * RECORDS_UNIT > payload.numel():
        raise PackedArenaFull(f'the packed records need {(unit_offset + units) * RECORDS_UNIT} bytes, the arena holds {payload.numel()}', units)
    _call('eas_records_pack', 8 * n + 8 * nb + RECORDS_UNIT * units, _lib.lib().eas_records_pack, ptr(rec), n, int(H), int(W), ptr(table_out),
          ptr(payload), unit_offset, unit_offset + units, stream())
    return units


def records_unpack(table, payload, a, e, H, W, return_flags=False):
    """The inverse of ``records_pack``: the logical records [a, e) of the store ``table`` int32 [NB, 2] / ``payload`` uint8 [used bytes] as
    8-byte records, uint8 [8 * (e - a)], byte for byte what was packed (padding included where the range covers it).  ``a < 0``, ``e < a``
    or ``e > 64 * NB`` raises ValueError.  ``return_flags``: also int32 [1], bit 1 set when a table entry placed a block outside the payload
    (those records come out as zeros)."""
    records_widths(H, W)
    nb, units = _packed_records_args(table, payload)
    a, e = int(a), int(e)
    if a < 0 or e < a or e > nb * RECORDS_BLOCK:
        raise ValueError(f'records_unpack: [{a}, {e}) is no range of {nb * RECORDS_BLOCK} packed records')
    out = torch.empty(8 * (e - a), dtype=torch.uint8, device=table.device)
    flags = torch.zeros(1, dtype=torch.int32, device=table.device) if return_flags else None
    if e > a:
        _call('eas_records_unpack', 12 * (e - a), _lib.lib().eas_records_unpack, ptr(table), nb, ptr(payload), units, a, e, int(H), int(W), ptr(out),
              ptr(flags), stream())
    return (out, flags) if return_flags else out


def _packed_ranges_frames(entry, dtype, out_bytes, table, payload, ranges, ns, H, W, tau, return_oob, return_flags):
    """the two packed-range wrappers: checks, allocations, the call (``tau``: a tuple, empty for the counts) and the return tuple"""
    records_widths(H, W)
    nb, units = _packed_records_args(table, payload)
    _dev(ranges)
    assert ranges.dtype == torch.int64 and ranges.dim() == 2 and ranges.shape[1] == 2 and ranges.device == table.device
    B = ranges.shape[0]
    out = torch.empty((B, ns, 2, H, W), dtype=dtype, device=table.device)
    oob = torch.empty(1, dtype=torch.int32, device=table.device) if return_oob else None
    flags = torch.empty(1, dtype=torch.int32, device=table.device) if return_flags else None
    # bytes: at most the table and the payload once + the frames
    _call(entry, 8 * nb + RECORDS_UNIT * units + out_bytes * out.numel(), getattr(_lib.lib(), entry), ptr(table) if nb else None, nb,
          ptr(payload) if units else None, units, ptr(ranges.contiguous()), B, ns, H, W, *tau, ptr(out), ptr(oob), ptr(flags), stream())
    ret = (out,) + ((oob,) if return_oob else ()) + ((flags,) if return_flags else ())
    return ret if len(ret) > 1 else out


def event_histogram_packed_ranges(table, payload, ranges, Tm, H, W, return_oob=False, return_flags=False):
    """``event_histogram_dat_ranges`` on packed records: ``table`` int32 [NB, 2] and ``payload`` uint8 [used bytes] (``records_pack``),
    ``ranges`` int64 [B, 2] of LOGICAL record indices -> count frames int32 [B, Tm, 2, H, W], bit-identical to ``event_histogram_dat_ranges``
    on the records that were packed.  Nothing is read back (graph-capturable).  Optional returns, in this order: the events outside the
    sensor that were dropped (int32 [1]); the flags (int32 [1], written by the call): bit 0 a range with a < 0, e > 64 * NB or e < a -- zero
    frames --, bit 1 a table entry that places a block outside the payload -- its records are skipped."""
    return _packed_ranges_frames('eas_event_histogram_packed_ranges', torch.int32, 4, table, payload, ranges, Tm, H, W, (), return_oob, return_flags)


def event_latest_surface_packed_ranges(table, payload, ranges, num_slices, H, W, tau=50e3, return_oob=False, return_flags=False):
    """``event_latest_surface_dat_ranges`` on packed records (the arguments and optional returns of ``event_histogram_packed_ranges``):
    float64 [B, num_slices, 2, H, W], bit-identical to that operator on the records that were packed"""
    return _packed_ranges_frames('eas_event_latest_surface_packed_ranges', torch.float64, 24, table, payload, ranges, num_slices, H, W,
                                 (float(tau),), return_oob, return_flags)


def label_targets(boxes, group_start, group, params, ih, iw, h, w, perm=None, max_labels=50, return_info=False):
    """The label side of a training batch from a box table in HBM: ``targets`` fp32 [B, max_labels, 5] rows (cls, cx, cy, w, h), zero padded --
    the box half of get_random_data (gen1.py:437, 459-468, 510-521), ``reformat('cxcywh')`` and EventTrainTransform for every sample in one
    launch (``data.transform_boxes`` + centre form + padding).  ``boxes`` fp32 [L, 5] rows (x1, y1, x2, y2, class) on the ``ih`` x ``iw``
    sensor; ``group_start`` int64 [G + 1]: rows group_start[g] .. group_start[g + 1] are label group g; ``group`` int64 [B]; ``params`` int32
    [B, 5] = (nw, nh, dx, dy, flip) on the ``h`` x ``w`` canvas; ``perm`` int32 [B, P] (None: identity): row j of a sample's shuffled list is
    row perm[b, j] of its group.  ``return_info``: also ``count`` int32 [B] (survivors before the cut at ``max_labels``) and ``flags`` int32
    [B] (bit 0: a perm entry outside the group, row dropped; bit 1: more rows than P, the rest dropped; bit 2: group outside [0, G), no
    rows).  Nothing is read back (graph-capturable)."""
    _dev(boxes, group_start, group, params, perm)
    assert boxes.dtype == torch.float32 and boxes.dim() == 2 and boxes.shape[1] == 5
    assert group_start.dtype == torch.int64 and group_start.dim() == 1 and group_start.numel() >= 1
    assert group.dtype == torch.int64 and group.dim() == 1
    B = group.numel()
    assert params.dtype == torch.int32 and params.shape == (B, 5)
    boxes, group_start, group, params = boxes.contiguous(), group_start.contiguous(), group.contiguous(), params.contiguous()
    P = 0
    if perm is not None:
        assert perm.dtype == torch.int32 and perm.dim() == 2 and perm.shape[0] == B
        perm, P = perm.contiguous(), perm.shape[1]
    targets = torch.empty((B, max_labels, 5), dtype=torch.float32, device=group.device)
    count = torch.empty(B, dtype=torch.int32, device=group.device) if return_info else None
    flags = torch.empty(B, dtype=torch.int32, device=group.device) if return_info else None
    # bytes: at most P (or every) row of each group once + the targets
    _call('eas_label_targets', 4 * targets.numel() + 24 * B * max(P, 1), _lib.lib().eas_label_targets, ptr(boxes), boxes.shape[0], ptr(group_start),
          group_start.numel() - 1, ptr(group), ptr(params), ptr(perm), P, B, int(ih), int(iw), int(h), int(w), int(max_labels), ptr(targets),
          ptr(count), ptr(flags), stream())
    return (targets, count, flags) if return_info else targets


def counts_to_canvas(counts, Hc, Wc):
    """int32 [..., H, W] -> float32 [..., Hc, Wc], zero padded bottom/right."""
    _dev(counts)
    assert counts.dtype == torch.int32
    counts = counts.contiguous()
    H, W = counts.shape[-2:]
    F = counts.numel() // (H * W)
    out = torch.empty(counts.shape[:-2] + (Hc, Wc), dtype=torch.float32, device=counts.device)
    check(_lib.lib().eas_counts_to_canvas(ptr(counts), F, H, W, Hc, Wc, ptr(out), stream()), 'eas_counts_to_canvas')
    return out


def counts_letterbox(counts, params, Hc, Wc, interp='linear'):
    """int32 counts [B, ..., H, W] -> fp32 [B, ..., Hc, Wc]: per-sample resize to (nw, nh) -- cv2 INTER_LINEAR semantics (Gen1), or
    ``interp='cubic'``: cv2 INTER_CUBIC (N-Caltech101) --, paste at (dx, dy), optional left-right flip; ``params`` int32 [B, 5] =
    (nw, nh, dx, dy, flip) (see data.letterbox_params / jitter_params)."""
    _dev(counts, params)
    assert counts.dtype == torch.int32 and params.dtype == torch.int32 and params.shape == (counts.shape[0], 5)
    counts, params = counts.contiguous(), params.contiguous()
    B, (H, W) = counts.shape[0], counts.shape[-2:]
    F = counts.numel() // (B * H * W)
    out = torch.empty(counts.shape[:-2] + (Hc, Wc), dtype=torch.float32, device=counts.device)
    check(_lib.lib().eas_counts_letterbox_ex(ptr(counts), ptr(params), ('linear', 'cubic').index(interp), B, F, H, W, Hc, Wc, ptr(out), stream()),
          'eas_counts_letterbox_ex')
    return out


def frames_letterbox(frames, params, Hc, Wc, interp='linear'):
    """``counts_letterbox`` for float64 frames [B, ..., H, W] (``event_timesurface_atis``) -> fp32 [B, ..., Hc, Wc]: the same kernel body on a
    double source, so frames that hold integers give exactly what their int32 counts give."""
    _dev(frames, params)
    assert frames.dtype == torch.float64 and params.dtype == torch.int32 and params.shape == (frames.shape[0], 5)
    frames, params = frames.contiguous(), params.contiguous()
    B, (H, W) = frames.shape[0], frames.shape[-2:]
    F = frames.numel() // (B * H * W)
    out = torch.empty(frames.shape[:-2] + (Hc, Wc), dtype=torch.float32, device=frames.device)
    check(_lib.lib().eas_frames_letterbox_f64(ptr(frames), ptr(params), ('linear', 'cubic').index(interp), B, F, H, W, Hc, Wc, ptr(out), stream()),
          'eas_frames_letterbox_f64')
    return out


def event_voxel_grid(t, x, y, p, sample_offsets, n_bins, H, W):
    """float64 [B, n_bins, 1, H, W] bilinear-in-time voxel grid."""
    _dev(t, x, y, p, sample_offsets)
    B = sample_offsets.numel() - 1
    out = torch.empty((B, n_bins, 1, H, W), dtype=torch.float64, device=t.device)
    check(_lib.lib().eas_event_voxel_grid(ptr(t), ptr(x), ptr(y), ptr(p), t.numel(), ptr(sample_offsets), B, n_bins, H, W,
                                          ptr(out), stream()), 'eas_event_voxel_grid')
    return out


def event_voxel_cube(t, x, y, p, sample_offsets, num_slices, H, W, tbins=2):
    """int32 [B, num_slices, 2*tbins, H, W] voxel-cube counts (the reference returns them as float64)."""
    _dev(t, x, y, p, sample_offsets)
    B = sample_offsets.numel() - 1
    out = torch.empty((B, num_slices, 2 * tbins, H, W), dtype=torch.int32, device=t.device)
    check(_lib.lib().eas_event_voxel_cube(ptr(t), ptr(x), ptr(y), ptr(p), t.numel(), ptr(sample_offsets), B, num_slices, tbins, H, W,
                                          ptr(out), stream()), 'eas_event_voxel_cube')
    return out


def event_time_surface(t, x, y, p, sample_offsets, num_slices, H, W, tau=50e3):
    """float64 [B, num_slices, 2, H, W] exponential time surfaces at the end of every micro-slice."""
    _dev(t, x, y, p, sample_offsets)
    B = sample_offsets.numel() - 1
    ws = torch.empty((B, num_slices, 2, H, W), dtype=torch.int32, device=t.device)
    out = torch.empty((B, num_slices, 2, H, W), dtype=torch.float64, device=t.device)
    check(_lib.lib().eas_event_time_surface(ptr(t), ptr(x), ptr(y), ptr(p), t.numel(), ptr(sample_offsets), B, num_slices, H, W,
                                            float(tau), ptr(ws), ptr(out), stream()), 'eas_event_time_surface')
    return out
