"""The detection-loss and SimOTA kernels (csrc/detloss.hip, csrc/simota.hip) against the fp64 restatement of tests/detloss_ref.py, its
gradients by torch.autograd.  Kernels are called through the C ABI where a case needs a hand-made assignment or a return code, through
ops.* otherwise; every output is pre-filled with NaN / 99, so an element that is not written fails.

Error bars: none is a constant.  For each quantity the bar is 4 x the worst error of the float32 tensor-op form (the mirror's
YOLOXHead._assign / get_losses with fused_loss = fused_assign = False / decode_outputs, run on the device on the same inputs) against
the same fp64 reference, with a floor of 8 * 2^-24 * (1 + |ref|) where that form happens to be exact; never taken from the kernel's own
output.  4: the kernels add in another order (float32 per thread, then doubles, then a fixed-order finalize), so their rounding is of
the same size, not of the same value.  Values are measured as |x - ref| / (1 + |ref|), gradient maps as |x - ref| / max|ref| of the map.

The assignment is discrete: on images the reference calls DECIDED (detloss_ref.assign) fg and matched must be identical; on undecided
ones the invariants that hold either way are checked.  tests/test_cpu_detloss_ref.py asserts, for the same seeds and shapes and without
a GPU, that at most 5 % of a case's labelled images are undecided.

Groups: A eas_det_labels | B eas_det_decode, eas_det_decode_eval | C eas_simota_assign, eas_simota_assign_rows | D eas_det_loss with
hand-made assignments, and its grid-stride wrap | E the whole path ops.det_loss and its backward."""
import ctypes as C

import pytest
import torch

import detloss_ref as dr

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -2                         # include/eas_hip.h: EAS_ERR_UNSUPPORTED
NAN = float('nan')
WORST, UNDECIDED = {}, {}                  # per group: (error, bar) of the comparison closest to its bar; per case: largest undecided share
_REFS = {}                                 # the fp64 references, computed once per case and shared by the tests that need them


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    import eas_snn_amd
    eas_snn_amd.hip_library()          # fail loudly if the extension is missing
    yield torch.device('cuda:0')
    for g in sorted(WORST):
        print(f'\ndetection loss, group {g}: worst error {WORST[g][0]:.3g} (bar {WORST[g][1]:.3g})', end='')
    for c in sorted(UNDECIDED):
        print(f'\ndetection loss, case {c}: largest undecided share {UNDECIDED[c]:.3g}', end='')


# ------------------------------------------------------------------------------------------------ comparisons
def _record(group, err, bar):
    if err != err:
        WORST[group] = (NAN, bar)
    elif group not in WORST or (WORST[group][0] == WORST[group][0] and err / bar > WORST[group][0] / WORST[group][1]):
        WORST[group] = (err, bar)


def _check_values(group, what, got, tens, ref):
    """got (the kernel) and tens (the float32 tensor-op form) against ref (fp64), all of one shape"""
    got, tens, ref = got.detach().double().cpu(), tens.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape == tens.shape, what
    if ref.numel() == 0:
        return
    err = float(((got - ref).abs() / (1 + ref.abs())).max())
    bar = max(4 * float(((tens - ref).abs() / (1 + ref.abs())).max()), dr.FLOOR)
    print(f'{group} {what}: error {err:.3g}, bar {bar:.3g}')
    _record(group, err, bar)
    assert err <= bar, f'{what}: error {err:.3g} above the bar {bar:.3g}'       # NaN (a sentinel left behind) fails


def _check_map(group, what, got, tens, ref):
    """a gradient map, relative to max|ref| of the map; a map that is zero in the reference must be exactly zero"""
    got, tens, ref = got.detach().double().cpu(), tens.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape == tens.shape, what
    assert not bool(torch.isnan(got).any()), f'{what}: a NaN sentinel is left in the map'
    m = float(ref.abs().max())
    if m == 0.0:
        assert not bool(got.any()), f'{what}: the reference map is zero, the kernel\'s is not'
        return
    err = float((got - ref).abs().max()) / m
    bar = max(4 * float((tens - ref).abs().max()) / m, dr.FLOOR * (1 + m) / m)
    print(f'{group} {what}: error {err:.3g}, bar {bar:.3g}')
    _record(group, err, bar)
    assert err <= bar, f'{what}: error {err:.3g} above the bar {bar:.3g}'


# ------------------------------------------------------------------------------------------------ launchers (sentinels in every output)
def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _geom_args(regs, strides):
    hws = [tuple(r.shape[-2:]) for r in regs]
    return hws, (C.c_int * (2 * len(hws)))(*[v for hw in hws for v in hw]), (C.c_float * len(hws))(*[float(s) for s in strides])


def _c_decode(regs, objs, clss, strides, sig, expect=0):
    from eas_snn_amd import _lib, ops
    hws, hw_arr, st_arr = _geom_args(regs, strides)
    B, nc = regs[0].shape[0], clss[0].shape[1]
    dec = torch.full((B, sum(h * w for h, w in hws), 5 + nc), NAN, device=regs[0].device)
    fn = _lib.lib().eas_det_decode_eval if sig else _lib.lib().eas_det_decode
    rc = fn(len(regs), _ptrs(regs), _ptrs(objs), _ptrs(clss), hw_arr, st_arr, B, nc, ops.ptr(dec), ops.stream())
    assert rc == expect, f'decode returned {rc}, expected {expect}'
    return dec


def _c_labels(lab, expect=0):
    from eas_snn_amd import _lib, ops
    B, G = lab.shape[:2]
    gv = torch.full((B, G), 99, dtype=torch.uint8, device=lab.device)
    gc, gb, n = torch.full((B, G), NAN, device=lab.device), torch.full((B, G, 4), NAN, device=lab.device), torch.full((), NAN, device=lab.device)
    rc = _lib.lib().eas_det_labels(ops.ptr(lab), B, G, ops.ptr(gv), ops.ptr(gc), ops.ptr(gb), ops.ptr(n), ops.stream())
    assert rc == expect, f'eas_det_labels returned {rc}, expected {expect}'
    return gv, gc, gb, n


def _c_simota(grids, svec, gt_boxes, gt_cls, gt_valid, bbox, obj, cls, rows, expect=0):
    """eas_simota_assign on separate arrays, or (rows) eas_simota_assign_rows on one decoded buffer [B, A, 5 + nc] built from them"""
    from eas_snn_amd import _lib, ops
    B, A = bbox.shape[:2]
    G, nc = gt_valid.shape[1], cls.shape[-1]
    dev_ = bbox.device
    fg = torch.full((B, A), 99, dtype=torch.uint8, device=dev_)
    matched = torch.full((B, A), 99, dtype=torch.int64, device=dev_)
    miou = torch.full((B, A), NAN, device=dev_)
    gv = gt_valid.to(torch.uint8).contiguous()
    p = ops.ptr
    if rows:
        dec = torch.cat([bbox, obj[..., None], cls], -1).contiguous()
        rc = _lib.lib().eas_simota_assign_rows(p(grids), p(svec), p(gt_boxes), p(gt_cls), p(gv), p(dec), B, G, A, nc, p(fg), p(matched), p(miou),
                                               ops.stream())
    else:
        rc = _lib.lib().eas_simota_assign(p(grids), p(svec), p(gt_boxes), p(gt_cls), p(gv), p(bbox), p(obj), p(cls), B, G, A, nc, p(fg), p(matched),
                                          p(miou), ops.stream())
    assert rc == expect, f'simota returned {rc}, expected {expect}'
    return fg, matched, miou


def _c_loss(regs, objs, clss, strides, dec, gt_boxes, gt_cls, fg, matched, miou, num_gts, use_l1):
    """eas_det_loss -> (out [7], gradient maps per level (g_reg, g_obj, g_cls) holding d(total * num_fg) / d(raw))"""
    from eas_snn_amd import _lib, ops
    lib = _lib.lib()
    hws, hw_arr, st_arr = _geom_args(regs, strides)
    B, nc, G = regs[0].shape[0], clss[0].shape[1], gt_cls.shape[1]
    g_regs, g_objs, g_clss = [[torch.full_like(t, NAN) for t in ts] for ts in (regs, objs, clss)]
    out = torch.full((7,), NAN, device=dec.device)
    ws = torch.empty(lib.eas_det_loss_workspace_doubles(), dtype=torch.float64, device=dec.device)
    p = ops.ptr
    ops.check(lib.eas_det_loss(len(regs), _ptrs(regs), _ptrs(objs), _ptrs(clss), _ptrs(g_regs), _ptrs(g_objs), _ptrs(g_clss), hw_arr, st_arr, B, nc,
                               p(dec), p(gt_boxes), p(gt_cls), G, p(fg), p(matched), p(miou), p(num_gts), int(use_l1), p(out), p(ws), ops.stream()),
              'eas_det_loss')
    return out, list(zip(g_regs, g_objs, g_clss))


# ------------------------------------------------------------------------------------------------ the float32 tensor-op form (the bars)
def _head(nc, strides):
    from yolox.models.yolo_head import YOLOXHead
    head = YOLOXHead(nc, width=1 / 32, strides=list(strides), in_channels=[256] * len(strides))
    head.fused_assign = head.fused_loss = False
    return head


def _tensor_decode(regs, objs, clss, strides, sig):
    """the head's own tensor operators: training rows (yolo_head.py forward) or the inference output (assemble_eval / decode_outputs)"""
    from yolox.models.yolo_head import _grid
    head = _head(clss[0].shape[1], strides)
    if sig:
        outputs = [torch.cat([r, o.sigmoid(), c.sigmoid()], 1) for r, o, c in zip(regs, objs, clss)]
        head.hw = [o.shape[-2:] for o in outputs]
        out = torch.cat([o.flatten(start_dim=2) for o in outputs], dim=2).permute(0, 2, 1)
        return head.decode_outputs(out, dtype=out.type())
    outs = []
    for r, o, c, s in zip(regs, objs, clss, strides):
        out = torch.cat([r, o, c], 1)
        grid = _grid(out.shape[-2], out.shape[-1], out.device, out.dtype)
        out = out.flatten(2).permute(0, 2, 1)
        outs.append(torch.cat([(out[..., :2] + grid) * s, torch.exp(out[..., 2:4]) * s, out[..., 4:]], -1))
    return torch.cat(outs, 1)


def _tensor_loss(regs, objs, clss, lab, strides, use_l1, assignment=None, scale=1.0):
    """get_losses of the mirror in float32 on the device, with its own _assign or a given assignment
    -> (six values, gradient maps per level of scale * total, (fg, matched, matched_iou) it used)"""
    from yolox.models.yolo_head import _grid
    L, nc = len(regs), clss[0].shape[1]
    head = _head(nc, strides)
    head.use_l1 = use_l1
    used = []
    if assignment is not None:
        head._assign = lambda *a: assignment
    else:
        inner = head._assign
        head._assign = lambda *a: used.append(inner(*a)) or used[0]
    leaves = [t.detach().clone().requires_grad_(True) for t in list(regs) + list(objs) + list(clss)]
    outs, origin, grids, svec = [], [], [], []
    for r, o, c, s in zip(leaves[:L], leaves[L:2 * L], leaves[2 * L:], strides):
        out = torch.cat([r, o, c], 1)
        grid = _grid(out.shape[-2], out.shape[-1], out.device, out.dtype)
        out = out.flatten(2).permute(0, 2, 1)
        outs.append(torch.cat([(out[..., :2] + grid) * s, torch.exp(out[..., 2:4]) * s, out[..., 4:]], -1))
        grids.append(grid)
        svec.append(torch.full((1, grid.shape[1]), float(s), device=out.device, dtype=out.dtype))
        origin.append(r.flatten(2).permute(0, 2, 1))
    vals = head.get_losses(torch.cat(grids, 1), torch.cat(svec, 1), lab, torch.cat(outs, 1), torch.cat(origin, 1) if use_l1 else None)
    gr = torch.autograd.grad(scale * vals[0], leaves)
    vals = [torch.as_tensor(v, dtype=torch.float32).detach() for v in vals]
    return vals, [(gr[l], gr[L + l], gr[2 * L + l]) for l in range(L)], (assignment if assignment is not None else used[0])


def _dv(dev, *ts):
    return [t.to(dev) for t in ts]


# ================================================================================================ A. labels
def _draw_labels(B, G, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.zeros(B, G, 5)
    n = torch.randint(0, G + 1, (B,), generator=g)
    if B > 1:
        n[0] = 0                                             # an image with no rows
    n[-1] = G                                                # and a full one
    rows = torch.cat([torch.randint(0, 3, (B, G, 1), generator=g).float(), torch.rand(B, G, 4, generator=g) * 90 + 1], -1)   # class 0 included
    lab = torch.where((torch.arange(G)[None] < n[:, None])[..., None], rows, lab)
    for b in range(B):
        if b % 3 == 1 and n[b] >= 3:
            lab[b, 1] = 0.0                                  # an all-zero row in the middle of the valid rows
    return lab


@pytest.mark.parametrize('G', [1, 50, 255])
@pytest.mark.parametrize('B', [1, 255, 256, 257, 1024])
def test_labels_are_bit_exact(dev, B, G):
    lab = _draw_labels(B, G, 100 + B + G)
    gv_r, gc_r, gb_r, n_r = dr.labels(lab.double())
    if B >= 255 and G >= 50:
        assert bool((lab[:, 1].sum(-1) == 0)[(lab.sum(-1) > 0).sum(-1) >= 2].any()), 'the draw holds a zero row among valid rows'
    gv, gc, gb, n = _c_labels(lab.to(dev))
    assert torch.equal(gv.cpu(), gv_r.to(torch.uint8)), 'gt_valid'
    assert torch.equal(gc.cpu().double(), gc_r) and torch.equal(gb.cpu().double(), gb_r), 'gt_cls / gt_boxes'
    assert float(n) == float(n_r), 'num_gts'


def test_labels_beyond_1024_images(dev):
    """eas_det_labels refuses B = 1025 before any launch; ops.det_loss then prepares the labels with tensor operators and gives, on the
    shared images, what it gives for B = 1024 (the extra image has no label, so num_fg and every per-anchor term are the same)"""
    from eas_snn_amd import _lib, ops
    lab = torch.zeros(1025, 4, 5)
    lab[:1024] = _draw_labels(1024, 4, 7)
    rows = lab[:1024].sum(-1, keepdim=True) > 0
    lab[:1024, :, 1:3] = torch.where(rows, lab[:1024, :, 1:3] * 0.3 + 4, torch.zeros(()))      # centres on the 24 x 40 canvas
    before = _lib.lib().eas_launch_counter()
    _c_labels(lab.to(dev), expect=E_UNSUPPORTED)
    assert _lib.lib().eas_launch_counter() == before, 'a refused call launched a kernel'
    g = torch.Generator().manual_seed(8)
    raw = [torch.randn(1025, c, 3, 5, generator=g) * 0.5 for c in (4, 1, 2)]
    res = []
    for B in (1024, 1025):
        leaves = [t[:B].to(dev).requires_grad_(True) for t in raw]
        out = ops.det_loss([leaves[0]], [leaves[1]], [leaves[2]], lab[:B].to(dev), [8], 2, True)
        out[0].backward()
        res.append(([float(v.detach()) for v in out], [t.grad[:1024].clone() for t in leaves]))
    (v0, g0), (v1, g1) = res
    assert v0[5] == v1[5] and v0[5] > 0
    for i in (1, 3, 4):                                      # sums over the foreground anchors only: the same terms
        assert abs(v0[i] - v1[i]) <= dr.FLOOR * (1 + abs(v0[i])), (i, v0[i], v1[i])
    assert v1[2] > v0[2]                                     # the objectness term of the extra image
    for a, b in zip(g0, g1):
        assert torch.equal(a, b) and not bool(torch.isnan(a).any())


# ================================================================================================ B. decode
DECODE_GEOMS = {'one-level': ([(3, 5)], [8], 2, 3), 'four-levels': ([(5, 7), (3, 4), (2, 2), (1, 3)], [8, 16, 32, 64], 3, 2),
                'wrap': ([(128, 128)], [8], 129, 1)}      # (levels, strides, B, nc); wrap: B * A = 2113536 > 8192 blocks * 256 threads


def _draw_raw(hws, B, nc, seed):
    g = torch.Generator().manual_seed(seed)
    return ([torch.randn(B, 4, h, w, generator=g) * 0.6 for h, w in hws], [torch.randn(B, 1, h, w, generator=g) * 2 for h, w in hws],
            [torch.randn(B, nc, h, w, generator=g) * 2 for h, w in hws])


@pytest.mark.parametrize('sig', [False, True], ids=['train', 'eval'])
@pytest.mark.parametrize('geom', list(DECODE_GEOMS))
def test_decode(dev, geom, sig):
    hws, strides, B, nc = DECODE_GEOMS[geom]
    regs, objs, clss = _draw_raw(hws, B, nc, 11)
    ref = dr.decode(*[dr.to64(*ts) for ts in (regs, objs, clss)], strides, sig)
    d_regs, d_objs, d_clss = _dv(dev, *regs), _dv(dev, *objs), _dv(dev, *clss)
    got = _c_decode(d_regs, d_objs, d_clss, strides, sig).cpu()
    tens = _tensor_decode(d_regs, d_objs, d_clss, strides, sig).cpu()
    for name, sl in (('cx', slice(0, 1)), ('cy', slice(1, 2)), ('w', slice(2, 3)), ('h', slice(3, 4)), ('obj', slice(4, 5)), ('cls', slice(5, None))):
        _check_values('B', f'{geom} sig={sig} {name}', got[..., sl], tens[..., sl], ref[..., sl])
    a0 = 0
    for h, w in hws:                                         # explicitly: the anchors on either side of every level start
        for a in sorted({max(a0 - 1, 0), a0, a0 + h * w - 1}):
            _check_values('B', f'{geom} sig={sig} anchor {a}', got[:, a], tens[:, a], ref[:, a])
        a0 += h * w
    if geom != 'wrap':
        from eas_snn_amd import ops
        if sig:
            via_ops = ops.det_decode_eval(list(zip(d_regs, d_objs, d_clss)), strides, nc)
            assert torch.equal(via_ops.cpu(), got)


# ================================================================================================ C. SimOTA
def _simota_ref(case):
    key = ('simota', case[0])
    if key not in _REFS:
        d = dr.draw_simota(case)
        _REFS[key] = (d, dr.assign_case(d))
    return _REFS[key]


def _pair_iou64(d, b, matched, fg):
    """fp64 IoU of every foreground anchor of image b with the row it is matched to"""
    gb, bx = d['gt_boxes'][b].double(), d['bbox'][b].double()
    a = fg.nonzero().flatten()
    return torch.stack([dr.pair_iou(gb[matched[i]][None], bx[i][None])[0, 0] for i in a]) if a.numel() else torch.zeros(0, dtype=torch.float64)


@pytest.mark.parametrize('rows', [False, True], ids=['arrays', 'rows'])
@pytest.mark.parametrize('case', dr.SIMOTA_CASES, ids=[c[0] for c in dr.SIMOTA_CASES])
def test_simota(dev, case, rows):
    d, (fg_r, m_r, iou_r, info) = _simota_ref(case)
    names = ('grids', 'strides', 'gt_boxes', 'gt_cls', 'gt_valid', 'bbox', 'obj', 'cls')
    args = _dv(dev, *[d[k] for k in names])
    fg, matched, miou = _c_simota(*args, rows)
    if d['grids'].shape[0] > 4096:                           # the parked state must not leak: a second run gives the same bits
        fg2, matched2, miou2 = _c_simota(*args, rows)
        assert torch.equal(fg, fg2) and torch.equal(matched, matched2) and torch.equal(miou.view(torch.int32), miou2.view(torch.int32))
    if not rows:
        from eas_snn_amd import ops
        o_fg, o_m, o_iou = ops.simota_assign(args[0][None], args[1][None], *args[2:6], args[6][..., None], args[7])
        assert torch.equal(o_fg, fg.bool()) and torch.equal(o_m, matched) and torch.equal(o_iou.view(torch.int32), miou.view(torch.int32))
    fg_t, m_t, iou_t = _head(d['nc'], [8])._assign(args[0][None], args[1][None], *args[2:6], args[6][..., None], args[7])
    fg, matched, miou, fg_t, m_t, iou_t = fg.cpu(), matched.cpu(), miou.cpu(), fg_t.cpu(), m_t.cpu(), iou_t.cpu()
    assert bool(((fg == 0) | (fg == 1)).all()), 'fg holds something that is neither 0 nor 1 (a sentinel left behind)'
    fg = fg.bool()
    assert not bool(torch.isnan(miou).any())
    assert bool((matched[~fg] == 0).all()) and bool((miou[~fg] == 0).all()), 'anchors that are not foreground carry 0 / 0.0'
    share, _ = dr.undecided_share(info)
    UNDECIDED[case[0]] = max(UNDECIDED.get(case[0], 0.0), share)
    got_iou, tens_iou, ref_iou = [], [], []
    G = d['gt_valid'].shape[1]
    for b, r in enumerate(info):
        if r['decided']:
            ndiff = int((fg[b] != fg_r[b]).sum())
            assert ndiff == 0, f'image {b}: foreground differs on {ndiff} anchors'
            assert torch.equal(matched[b][fg[b]], m_r[b][fg[b]]), f'image {b}: matched rows differ'
            assert torch.equal(fg_t[b], fg_r[b]) and torch.equal(m_t[b][fg[b]], m_r[b][fg[b]]), f'image {b}: the tensor form differs on a decided image'
            got_iou.append(miou[b]); tens_iou.append(iou_t[b]); ref_iou.append(iou_r[b])
        else:                                                # what holds whichever way the rounding fell
            assert not bool((fg[b] & ~r['cand']).any()), f'image {b}: foreground outside the candidates'
            m = matched[b][fg[b]]
            assert bool(((m >= 0) & (m < G)).all()) and bool(d['gt_valid'][b][m].all()), f'image {b}: matched to a row that is not valid'
            assert int(torch.bincount(m, minlength=G).max()) <= 10 if m.numel() else True, f'image {b}: a row owns more than 10 anchors'
            pair = _pair_iou64(d, b, matched[b], fg[b])
            got_iou.append(miou[b][fg[b]]); ref_iou.append(pair)
            # the tensor form's own pairs may differ here: its error on its own pairs is as good a measure of float32
            tens_iou.append(pair + (iou_t[b][fg_t[b]].double() - _pair_iou64(d, b, m_t[b], fg_t[b])).abs().max() if bool(fg_t[b].any()) and m.numel()
                            else pair)
    _check_values('C', f'{case[0]} rows={rows} matched_iou', torch.cat(got_iou), torch.cat(tens_iou), torch.cat(ref_iou))
    if case[2] == 'far':
        # image 2: its only row has no candidate anchor -> nothing.  image 3: the row far outside takes at most the one anchor its
        # dyn_k = 1 buys (the cheapest candidate of the OTHER rows, in the +1e6 range) and leaves those rows' anchors as they are
        assert not bool(fg[2].any())
        gv = d['gt_valid'].clone()
        gv[3, 3] = False
        a = dr.to64(d['grids'], d['strides'], d['gt_boxes'][3:4], d['gt_cls'][3:4], gv[3:4], d['bbox'][3:4], d['obj'][3:4], d['cls'][3:4])
        fg_w, m_w, _, info_w = dr.assign(*a, d['nc'])
        assert info_w[0]['decided']
        own = fg[3] & (matched[3] == 3)
        assert int(own.sum()) <= 1 and torch.equal(fg[3] & ~own, fg_w[0] & ~own) and torch.equal(matched[3][fg_w[0] & ~own], m_w[0][fg_w[0] & ~own])


def test_simota_refusals(dev):
    """A = 12289 and G = 256 are decided on the host: EAS_ERR_UNSUPPORTED, no launch, outputs untouched"""
    from eas_snn_amd import _lib, ops
    for B, G, A in ((1, 4, 12289), (1, 256, 16)):
        grids, svec = torch.zeros(A, 2, device=dev), torch.full((A,), 8.0, device=dev)
        gb, gc, gv = torch.ones(B, G, 4, device=dev), torch.zeros(B, G, device=dev), torch.ones(B, G, dtype=torch.bool, device=dev)
        bbox, obj, cls = torch.ones(B, A, 4, device=dev), torch.zeros(B, A, device=dev), torch.zeros(B, A, 2, device=dev)
        assert not ops.simota_supported(gv, bbox)
        for rows in (False, True):
            before = _lib.lib().eas_launch_counter()
            fg, matched, miou = _c_simota(grids, svec, gb, gc, gv, bbox, obj, cls, rows, expect=E_UNSUPPORTED)
            assert _lib.lib().eas_launch_counter() == before, 'a refused call launched a kernel'
            assert bool((fg == 99).all()) and bool((matched == 99).all()) and bool(torch.isnan(miou).all())
    assert ops.simota_supported(torch.ones(1, 255, dtype=torch.bool, device=dev), torch.ones(1, 12288, 4, device=dev))


# ================================================================================================ D. loss and gradient, hand-made assignments
HAND_GEOMS = {1: ([(3, 5)], [8]), 3: dr.GEOMS['c3'], 4: ([(5, 7), (3, 4), (2, 2), (1, 3)], [8, 16, 32, 64])}


def _hand_case(L, nc, seed, no_fg=False, tie=True):
    """raw maps, labels [3, 6, 5] with every row of images 1 and 2 valid, and an assignment made by hand.  Image 1, level 0: anchor 1
    ties on all four edges (raw reg 0, its row an s x s box on the decoded centre), anchor 2 has an empty intersection with its row,
    anchor 3 is matched to a row 1e-3 wide; rows 3 / 4 carry class ids -1 / nc + 3, row G - 1 is matched too; both anchors on either
    side of every level start are foreground; image 2 has large rows and a random third of its anchors foreground, each matched to the row
    nearest to its decoded centre, so that most pairs overlap.  ``tie`` False leaves anchor 1 background: with the L1 term its target
    log(s / s + 1e-8) is 0 in float32 and 1e-8 in float64, against a raw value of exactly 0 -- the sign of that difference is not a
    float32 question."""
    hws, strides = HAND_GEOMS[L]
    B, G = 3, 6
    g = torch.Generator().manual_seed(seed)
    regs, objs, clss = _draw_raw(hws, B, nc, seed)
    A = sum(h * w for h, w in hws)
    grids, svec = dr.anchors(hws, strides, torch.float32)
    ctr = grids * svec[:, None]
    lab = torch.zeros(B, G, 5)
    lab[0, :2] = torch.tensor([[0.0, 10, 10, 12, 9], [float(nc - 1), 20, 12, 8, 14]])
    for b in (1, 2):
        pick = torch.randint(0, A, (G,), generator=g)
        lab[b] = torch.cat([torch.randint(0, nc, (G, 1), generator=g).float(), ctr[pick] + torch.randn(G, 2, generator=g) * 3,
                            torch.rand(G, 2, generator=g) * (20 if b == 1 else 40) + (6 if b == 1 else 20)], 1)
    s0, W0 = float(strides[0]), hws[0][1]
    regs[0][1, :, 0, 1] = 0.0
    lab[1, 0, 1:] = torch.tensor([1 * s0, 0.0, s0, s0])                  # anchor 1 = pixel (x 1, y 0) of level 0
    lab[1, 0, 2] = 0.0
    lab[1, 1, 1:] = torch.tensor([1000.0, 1000.0, 10.0, 10.0])
    lab[1, 2, 1:] = torch.tensor([3 * s0 + 1.0, 2.0, 1e-3, 20.0])
    lab[1, 3, 0], lab[1, 4, 0] = -1.0, nc + 3.0
    assert W0 >= 4
    fg = torch.zeros(B, A, dtype=torch.bool)
    matched = torch.zeros(B, A, dtype=torch.int64)
    if not no_fg:
        edges, a0 = {0, A - 1}, 0
        for h, w in hws:
            edges |= {max(a0 - 1, 0), a0}
            a0 += h * w
        for b in (1, 2):
            for i, a in enumerate(sorted(edges)):
                fg[b, a], matched[b, a] = True, (G - 1, 3, 4, 5, 0)[(i + b) % 5]
        for a, m in ((1, 0), (2, 1), (3, 2))[0 if tie else 1:]:
            fg[1, a], matched[1, a] = True, m
        extra = torch.rand(A, generator=g) < 0.33
        dec_ctr = torch.cat([(r[2, :2].flatten(1).t() + dr.anchors([hw], [s], torch.float32)[0]) * s for r, hw, s in zip(regs, hws, strides)])
        nearest = (dec_ctr[:, None] - lab[2, None, :, 1:3]).pow(2).sum(-1).argmin(1)
        matched[2] = torch.where(extra & ~fg[2], nearest, matched[2])
        fg[2] |= extra
    miou = torch.where(fg, torch.rand(B, A, generator=g), torch.zeros(B, A))
    return regs, objs, clss, lab, strides, fg, matched, miou


def _run_hand(dev, group, what, regs, objs, clss, lab, strides, fg, matched, miou, use_l1):
    """eas_det_loss on a given assignment against detloss_ref.loss + autograd -> (out [7] on the host, kernel maps scaled by out[6])"""
    gv_r, gc_r, gb_r, n_r = dr.labels(lab.double())
    r64 = [dr.to64(*ts) for ts in (regs, objs, clss)]
    vals_r, grads_r = dr.loss_and_grads(*r64, gb_r, gc_r, n_r, fg, matched, miou.double(), strides, use_l1)
    d_regs, d_objs, d_clss = _dv(dev, *regs), _dv(dev, *objs), _dv(dev, *clss)
    d_lab, d_fg, d_m, d_iou = _dv(dev, lab, fg, matched, miou)
    gv, gc, gb, n = _c_labels(d_lab)
    dec = _c_decode(d_regs, d_objs, d_clss, strides, False)
    out, maps = _c_loss(d_regs, d_objs, d_clss, strides, dec, gb, gc, d_fg.to(torch.uint8), d_m, d_iou, n, use_l1)
    vals_t, grads_t, _ = _tensor_loss(d_regs, d_objs, d_clss, d_lab, strides, use_l1, assignment=(d_fg, d_m, d_iou))
    out = out.cpu()
    assert not bool(torch.isnan(out).any())
    for i, name in enumerate(('total', 'iou', 'obj', 'cls', 'l1', 'num_fg / num_gts')):
        _check_values(group, f'{what} {name}', out[i], vals_t[i], vals_r[i])
    assert float(out[6]) == float(torch.tensor(1.0) / max(float(fg.sum()), 1.0)), 'out[6] is the float32 quotient 1 / num_fg'
    scaled = []
    for l, (km, tm, rm) in enumerate(zip(maps, grads_t, grads_r)):
        scaled.append([k * out[6].to(dev) for k in km])
        for k, t, r, name in zip(scaled[-1], tm, rm, ('reg', 'obj', 'cls')):
            _check_map(group, f'{what} level {l} d{name}', k, t, r)
    return out, scaled, (vals_r, grads_r)


@pytest.mark.parametrize('L,nc,use_l1', [(1, 1, True), (1, 3, False), (3, 2, True), (3, 1, False), (4, 3, True), (4, 2, False)])
def test_loss_with_hand_made_assignment(dev, L, nc, use_l1):
    regs, objs, clss, lab, strides, fg, matched, miou = _hand_case(L, nc, 40 + L, tie=not use_l1)
    out, maps, (vals_r, grads_r) = _run_hand(dev, 'D', f'L={L} nc={nc} l1={use_l1}', regs, objs, clss, lab, strides, fg, matched, miou, use_l1)
    g_reg = maps[0][0].cpu()
    ref_reg = grads_r[0][0]
    if not use_l1:
        # the tie: IoU 1, every edge's gradient split in halves -- the two halves of a centre gradient cancel exactly
        assert float(ref_reg[1, 0, 0, 1]) == 0.0 and float(ref_reg[1, 1, 0, 1]) == 0.0
        assert float(g_reg[1, 0, 0, 1]) == 0.0 and float(g_reg[1, 1, 0, 1]) == 0.0
        # the empty intersection: IoU 0 and a box gradient of exactly 0
        assert not bool(g_reg[1, :, 0, 2].any()) and not bool(ref_reg[1, :, 0, 2].any())


@pytest.mark.parametrize('use_l1', [True, False])
def test_loss_without_any_foreground(dev, use_l1):
    regs, objs, clss, lab, strides, fg, matched, miou = _hand_case(3, 2, 50, no_fg=True)
    out, maps, (vals_r, _) = _run_hand(dev, 'D', f'no foreground l1={use_l1}', regs, objs, clss, lab, strides, fg, matched, miou, use_l1)
    num_gts = float(dr.labels(lab.double())[3])
    assert float(out[6]) == 1.0 and float(out[5]) == float(torch.tensor(1.0) / num_gts), 'no foreground counts as one: fmaxf(num_fg, 1)'
    assert float(out[0]) == float(out[2]) and float(out[1]) == float(out[3]) == float(out[4]) == 0.0
    for g_reg, _, g_cls in maps:
        assert not bool(g_reg.any()) and not bool(g_cls.any())


def _path_ref(case):
    key = ('path', case[0])
    if key not in _REFS:
        d = dr.draw_path(case)
        _REFS[key] = (d, dr.path_reference(d, need_grad=case is not dr.WRAP_CASE))
    return _REFS[key]


def test_loss_grid_stride_wrap(dev):
    """B * A = 65 * 4096 > 1024 blocks * 256 threads: the loss kernel's loop wraps.  The assignment comes from the SimOTA kernel on the
    decoded rows (and equals the reference's: the case is decided); the loss is compared for that assignment."""
    d, ref = _path_ref(dr.WRAP_CASE)
    strides, nc = d['strides'], d['nc']
    d_regs, d_objs, d_clss = _dv(dev, *d['regs']), _dv(dev, *d['objs']), _dv(dev, *d['clss'])
    gv, gc, gb, n = _c_labels(d['labels'].to(dev))
    dec = _c_decode(d_regs, d_objs, d_clss, strides, False)
    grids, svec = _dv(dev, *dr.anchors([tuple(r.shape[-2:]) for r in d['regs']], strides, torch.float32))
    from eas_snn_amd import _lib, ops
    B, A = dec.shape[:2]
    fg = torch.full((B, A), 99, dtype=torch.uint8, device=dev)
    matched, miou = torch.full((B, A), 99, dtype=torch.int64, device=dev), torch.full((B, A), NAN, device=dev)
    p = ops.ptr
    ops.check(_lib.lib().eas_simota_assign_rows(p(grids), p(svec), p(gb), p(gc), p(gv), p(dec), B, gv.shape[1], A, nc, p(fg), p(matched), p(miou),
                                                ops.stream()), 'eas_simota_assign_rows')
    assert torch.equal(fg.cpu().bool(), ref['fg']) and torch.equal(matched.cpu()[ref['fg']], ref['matched'][ref['fg']])
    _run_hand(dev, 'D', 'wrap', d['regs'], d['objs'], d['clss'], d['labels'], strides, fg.cpu().bool(), matched.cpu(), miou.cpu(), d['use_l1'])


# ================================================================================================ E. the whole path
@pytest.mark.parametrize('case', dr.PATH_CASES, ids=[c[0] for c in dr.PATH_CASES])
def test_whole_path(dev, case):
    from eas_snn_amd import ops
    d, ref = _path_ref(case)
    strides, nc, use_l1 = d['strides'], d['nc'], d['use_l1']
    L = len(d['regs'])
    lab = d['labels'].to(dev)
    assert ops.det_loss_supported(_dv(dev, *d['regs']), lab, 'iou')
    leaves = [t.to(dev).requires_grad_(True) for t in d['regs'] + d['objs'] + d['clss']]
    out = ops.det_loss(leaves[:L], leaves[L:2 * L], leaves[2 * L:], lab, strides, nc, use_l1)
    assert out[0].requires_grad and not any(o.requires_grad for o in out[1:])
    vals_t, grads_t, (fg_t, m_t, _) = _tensor_loss(leaves[:L], leaves[L:2 * L], leaves[2 * L:], lab, strides, use_l1, scale=3.5)
    assert torch.equal(fg_t.cpu(), ref['fg']) and torch.equal(m_t.cpu()[ref['fg']], ref['matched'][ref['fg']]), 'the tensor form on a decided batch'
    for i, name in enumerate(('total', 'iou', 'obj', 'cls', 'l1', 'num_fg / num_gts')):
        _check_values('E', f'{case[0]} {name}', out[i], vals_t[i], ref['values'][i])
    # a result that is not differentiable, used alone: nothing reaches the maps
    other = torch.zeros((), device=dev, requires_grad=True)
    (out[2] + out[5] + other).backward(retain_graph=True)
    assert all(t.grad is None for t in leaves) and float(other.grad) == 1.0
    first = torch.autograd.grad(3.5 * out[0], leaves, retain_graph=True)
    second = torch.autograd.grad(3.5 * out[0], leaves, retain_graph=True)
    for a, b in zip(first, second):
        assert torch.equal(a, b), 'a second backward through the retained graph gives another gradient'
    for l in range(L):
        for k, name in enumerate(('reg', 'obj', 'cls')):
            _check_map('E', f'{case[0]} level {l} d{name}', first[l + k * L], grads_t[l][k], 3.5 * ref['grads'][l][k])
