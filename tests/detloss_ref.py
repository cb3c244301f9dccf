"""Plain torch restatement, in float64, of what the detection-loss kernels compute (csrc/detloss.hip: eas_det_labels, eas_det_decode,
eas_det_decode_eval, eas_det_loss; csrc/simota.hip: eas_simota_assign, eas_simota_assign_rows), written term by term from the
per-image form of oracle/model_ref.py (YOLOXHead.forward / get_losses / get_assignments) and the loss terms of
compat/yolox/models/yolo_head.py get_losses.  Nothing here casts to float32: the tests feed it float32 values converted to float64.
There is no backward here: every gradient the tests compare with comes from torch.autograd on ``loss``.
tests/test_cpu_detloss_ref.py pins it to oracle.model_ref (which the goldens pin to the reference project) and to the mirror's
tensor-op form.

Two things the per-image original cannot express are taken from the batch-wide mirror, which the kernels follow: class ids outside
[0, nc) are clamped into it (F.one_hot would raise), and an image none of whose ground truths has an anchor inside its centre box has
no foreground (topk on an empty row would raise).

The second half holds the case lists and the seeded input draws that tests/test_gpu_detloss.py runs on the device and for which
tests/test_cpu_detloss_ref.py asserts the conditions the device comparison relies on: one definition, so the two cannot drift."""
import math

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24           # half a float32 ulp of 1: the relative error bound of one correctly rounded float32 operation
FLOOR = 8 * EPS            # floor of every error bar, times (1 + |ref|)
CAP_UNDECIDED = 0.05       # share of the labelled images of a case that may be undecided (and never all of them)

# In-centre test, on delta = xc - (gx - dist) and its three siblings.  The anchor centre xc = (i + 0.5) * s and dist = 1.5 * s are exact
# in float32 (small integers and halves), gx is a float32 input.  Two roundings remain: gx -+ dist, then the difference with xc, each at
# most EPS times a magnitude below |gx| + dist + xc <= about 4 * max(H, W) for a centre anywhere near the canvas (a centre far outside
# gives deltas far from zero): |error| <= 8 * EPS * max(H, W).  64 leaves a factor 8 above that bound.
K_CENTRE = 64
# Dynamic k, on the sum of the 10 largest IoUs.  One IoU is about 20 float32 operations (4 halvings that are exact, 8 corner sums, 4
# max / min that are exact, 2 side differences, 3 area products, 2 union sums, 1 division); the intersection sides cancel, but an IoU
# large enough to matter for the sum has sides comparable to the boxes, so each rounding stays a relative EPS of the result: <= 20 * EPS
# per IoU, carried unchanged into their sum, plus 9 additions of at most EPS * sum each -> 29 * EPS * sum.  32 is the next power of two.
K_DYNK = 32


def tau(nc):
    """Relative margin of a cost comparison.  The kernel's cost is a float32 sum: nc BCE terms added one after the other (nc roundings of
    a partial sum that never exceeds the cost), the product 3 * (-log(iou + 1e-8)) and its addition (2), the 1e6 term's product and its
    addition (2), and the rounding of the logarithm, square root, sigmoid and product feeding each BCE term (4, relative to a term that is
    below the cost): (nc + 8) roundings of at most EPS * |cost|.  With the 1e6 term present the margin is about 0.1 to 1 in absolute terms,
    which is where float32 (ulp 1/16) cannot decide."""
    return (nc + 8) * EPS


# ------------------------------------------------------------------------------------------------ anchors
def anchors(hws, strides, dtype=torch.float64):
    """grids [A, 2] (x, y) and strides [A] of the head levels, levels one after the other"""
    gs, ss = [], []
    for (h, w), s in zip(hws, strides):
        yv, xv = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        gs.append(torch.stack((xv, yv), 2).reshape(-1, 2).to(dtype))
        ss.append(torch.full((h * w,), float(s), dtype=dtype))
    return torch.cat(gs), torch.cat(ss)


# ------------------------------------------------------------------------------------------------ labels
def labels(lab):
    """labels [B, G, 5] (class, cx, cy, w, h; zero rows pad) -> gt_valid bool [B, G], gt_cls [B, G], gt_boxes [B, G, 4], num_gts (scalar).
    model_ref.py:281, 298-299: the number of rows whose five values sum to > 0 is COUNTED, then that many leading rows are taken."""
    nlabel = (lab.sum(dim=2) > 0).sum(dim=1)
    gt_valid = torch.arange(lab.shape[1])[None] < nlabel[:, None]
    return gt_valid, lab[:, :, 0].clone(), lab[:, :, 1:5].clone(), nlabel.sum().to(lab.dtype)


# ------------------------------------------------------------------------------------------------ decode
def decode(regs, objs, clss, strides, sig):
    """raw maps per level [B, 4 | 1 | nc, H, W] -> [B, A, 5 + nc]: (cx, cy, w, h, objectness, classes); model_ref.py:251-256 (training,
    logits) and :263-276 (inference, ``sig``: probabilities)"""
    outs = []
    for r, o, c, s in zip(regs, objs, clss, strides):
        H, W = r.shape[-2:]
        grid, _ = anchors([(H, W)], [s], r.dtype)
        if sig:
            o, c = o.sigmoid(), c.sigmoid()
        out = torch.cat([r, o, c], 1).flatten(2).permute(0, 2, 1)
        outs.append(torch.cat([(out[..., :2] + grid) * s, torch.exp(out[..., 2:4]) * s, out[..., 4:]], -1))
    return torch.cat(outs, 1)


# ------------------------------------------------------------------------------------------------ assignment
def pair_iou(gt, pred):
    """bboxes_iou of cxcywh boxes, gt [n, 4] x pred [m, 4] -> [n, m] (model_ref.py bboxes_iou_cxcywh; no epsilon in the denominator)"""
    a, b = gt[:, None, :], pred[None, :, :]
    tl = torch.maximum(a[..., :2] - a[..., 2:] / 2, b[..., :2] - b[..., 2:] / 2)
    br = torch.minimum(a[..., :2] + a[..., 2:] / 2, b[..., :2] + b[..., 2:] / 2)
    en = (tl < br).to(tl.dtype).prod(-1)
    area_i = (br - tl).prod(-1) * en
    return area_i / (a[..., 2:].prod(-1) + b[..., 2:].prod(-1) - area_i)


@torch.no_grad()
def assign(grids, strides, gt_boxes, gt_cls, gt_valid, bbox, obj, cls, nc):
    """SimOTA (model_ref.py:329-368) per image over its valid rows, in the dtype of the inputs (float64 in the tests).
    grids [A, 2], strides [A], gt_boxes [B, G, 4], gt_cls [B, G], gt_valid [B, G], bbox [B, A, 4], obj [B, A], cls [B, A, nc].
    -> fg bool [B, A], matched int64 [B, A] (label row, 0 where not fg), matched_iou [B, A], info: per image a dict with
    ``decided`` / ``reason`` / ``n`` (valid rows) / ``cand`` bool [A] / ``dyn_k`` (list) / ``multi`` (anchors claimed by several rows) /
    ``spill`` (rows with fewer anchors in their own centre box than dyn_k: they take anchors whose cost carries the 1e6 term).

    The assignment is discrete, so a float32 evaluation may differ from this one where a decision sits inside float32 rounding.  An
    image is UNDECIDED if any of these margins is too small (constants: K_CENTRE, K_DYNK, tau above, each derived by counting float32
    operations, none measured):
      in-centre test     some |min delta| < K_CENTRE * EPS * max(H, W)
      dyn_k              the sum of the top-10 IoUs is >= 0.5 and closer than K_DYNK * EPS * max(sum, 1) to an integer
      top-k cut          the dyn_k-th and (dyn_k+1)-th cheapest costs of a row differ by <= tau * |cost|
      multi-claim argmin the best and second-best cost of an anchor claimed by several rows differ by <= tau * |cost|
    The relative form of the last two widens to about 0.1 .. 1 where the cost carries the 1e6 term."""
    B, A = bbox.shape[:2]
    dt = bbox.dtype
    fg = torch.zeros((B, A), dtype=torch.bool)
    matched = torch.zeros((B, A), dtype=torch.int64)
    matched_iou = torch.zeros((B, A), dtype=dt)
    xc, yc, dist = (grids[:, 0] + 0.5) * strides, (grids[:, 1] + 0.5) * strides, strides * 1.5
    extent = float(((grids + 1) * strides[:, None]).max())
    t = tau(nc)
    info = []
    for b in range(B):
        rows = gt_valid[b].nonzero().flatten()
        n = int(rows.numel())
        rec = dict(decided=True, reason='', n=n, cand=torch.zeros(A, dtype=torch.bool), dyn_k=[], multi=0, spill=0)
        info.append(rec)
        if n == 0:
            continue
        why = []
        gb, gc = gt_boxes[b, rows], gt_cls[b, rows]
        gx, gy = gb[:, 0:1], gb[:, 1:2]
        deltas = torch.stack([xc - (gx - dist), yc - (gy - dist), (gx + dist) - xc, (gy + dist) - yc], 2)
        dmin = deltas.min(dim=-1).values                                   # [n, A]
        if bool((dmin.abs() < K_CENTRE * EPS * extent).any()):
            why.append('in-centre margin')
        in_centers = dmin > 0.0
        cand = in_centers.any(dim=0)
        rec['cand'] = cand
        ci = cand.nonzero().flatten()
        if ci.numel():
            ious = torch.zeros((n, A), dtype=dt)
            cost = torch.full((n, A), 1e12, dtype=dt)
            iou_c = pair_iou(gb, bbox[b, ci])
            onehot = F.one_hot(gc.to(torch.int64).clamp(0, nc - 1), nc).to(dt)
            joint = (cls[b, ci].sigmoid() * obj[b, ci].sigmoid()[:, None]).sqrt()
            cls_cost = F.binary_cross_entropy(joint[None].expand(n, -1, -1), onehot[:, None].expand(-1, ci.numel(), -1), reduction='none').sum(-1)
            ious[:, ci] = iou_c
            cost[:, ci] = cls_cost + 3.0 * (-torch.log(iou_c + 1e-8)) + 1e6 * (~in_centers[:, ci]).to(dt)
            ksum = torch.topk(ious, min(10, A), dim=1).values.sum(1)
            dyn_k = torch.clamp(ksum.to(torch.int64), min=1)
            rec['dyn_k'] = dyn_k.tolist()
            rec['spill'] = int((dyn_k > in_centers.sum(1)).sum())
            if bool(((ksum >= 0.5) & ((ksum - ksum.round()).abs() < K_DYNK * EPS * ksum.clamp(min=1.0))).any()):
                why.append('dyn_k margin')
            srt, order = torch.sort(cost, dim=1, stable=True)
            match = torch.zeros((n, A), dtype=torch.bool)
            for g in range(n):
                k = int(dyn_k[g])
                match[g, order[g, :k]] = True
                if k < A and srt[g, k - 1] < 1e12 and srt[g, k] - srt[g, k - 1] <= t * srt[g, k].abs():
                    why.append('top-k cut')
            match &= cand[None]
            per_anchor = match.sum(0)
            multi = per_anchor > 1
            rec['multi'] = int(multi.sum())
            if n > 1 and rec['multi']:
                two = torch.sort(cost[:, multi], dim=0).values[:2]
                if bool((two[1] - two[0] <= t * two[1].abs()).any()):
                    why.append('multi-claim argmin')
            best = cost.argmin(dim=0)                                       # first row of least cost
            which = torch.where(multi, best, match.to(torch.int8).argmax(0))
            f = per_anchor > 0
            fg[b] = f
            matched[b] = torch.where(f, rows[which], torch.zeros_like(which))
            matched_iou[b] = torch.where(f, ious[which, torch.arange(A)], torch.zeros((), dtype=dt))
        rec['decided'], rec['reason'] = not why, ', '.join(sorted(set(why)))
    return fg, matched, matched_iou, info


# ------------------------------------------------------------------------------------------------ loss
def loss(regs, objs, clss, gt_boxes, gt_cls, num_gts, fg, matched, matched_iou, strides, use_l1):
    """The six numbers of get_losses (model_ref.py:279-326: total, 5 * iou, obj, cls, l1, num_fg / num_gts) from the raw maps and a GIVEN
    assignment, as tensors of the maps' dtype with a graph: torch.autograd.grad gives the gradient maps.  A foreground anchor's class
    target is onehot(clamped class) * matched_iou, its box target the matched row."""
    nc = clss[0].shape[1]
    dt = regs[0].dtype
    dec = decode(regs, objs, clss, strides, sig=False)
    hws = [tuple(r.shape[-2:]) for r in regs]
    grids, svec = anchors(hws, strides, dt)
    origin = torch.cat([r.flatten(2).permute(0, 2, 1) for r in regs], 1)
    bi, ai = fg.nonzero(as_tuple=True)
    m = matched[bi, ai]
    num_fg = max(float(fg.sum()), 1.0)
    pred, target = dec[bi, ai, :4], gt_boxes[bi, m].to(dt)
    # iou_loss (model_ref.py:195-205)
    tl = torch.maximum(pred[:, :2] - pred[:, 2:] / 2, target[:, :2] - target[:, 2:] / 2)
    br = torch.minimum(pred[:, :2] + pred[:, 2:] / 2, target[:, :2] + target[:, 2:] / 2)
    area_p, area_g = pred[:, 2] * pred[:, 3], target[:, 2] * target[:, 3]
    en = (tl < br).to(dt).prod(dim=1)
    area_i = (br - tl)[:, 0] * (br - tl)[:, 1] * en
    iou = area_i / (area_p + area_g - area_i + 1e-16)
    loss_iou = (1 - iou ** 2).sum() / num_fg
    loss_obj = F.binary_cross_entropy_with_logits(dec[:, :, 4], fg.to(dt), reduction='none').sum() / num_fg
    cls_t = F.one_hot(gt_cls[bi, m].to(torch.int64).clamp(0, nc - 1), nc).to(dt) * matched_iou[bi, ai].to(dt)[:, None]
    loss_cls = F.binary_cross_entropy_with_logits(dec[bi, ai, 5:], cls_t, reduction='none').sum() / num_fg
    if use_l1:
        s = svec[ai]
        l1_t = torch.stack([target[:, 0] / s - grids[ai, 0], target[:, 1] / s - grids[ai, 1],
                            torch.log(target[:, 2] / s + 1e-8), torch.log(target[:, 3] / s + 1e-8)], 1)
        loss_l1 = (origin[bi, ai] - l1_t).abs().sum() / num_fg
    else:
        loss_l1 = torch.zeros((), dtype=dt)
    total = 5.0 * loss_iou + loss_obj + loss_cls + loss_l1
    ratio = torch.tensor(num_fg / max(float(num_gts), 1.0), dtype=dt)
    return total, 5.0 * loss_iou, loss_obj, loss_cls, loss_l1, ratio


def to64(*ts):
    return [t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu() for t in ts]


# ================================================================================================ cases and seeded draws
# head geometries: name -> (levels (H_l, W_l), strides)
GEOMS = {
    'a1': ([(1, 1)], [8]),                                   # one anchor
    'a9': ([(3, 3)], [8]),                                   # fewer anchors than the 10 of the top-k (kk = A)
    'c3': ([(8, 12), (4, 6), (2, 3)], [8, 16, 32]),          # the three-level 64 x 96 canvas, A = 126
    'c3b': ([(12, 16), (6, 8), (3, 4)], [8, 16, 32]),        # 96 x 128, A = 252
    'a4096': ([(64, 64)], [8]),                              # the largest small form (25 B of LDS per anchor)
    'a4097': ([(64, 64), (1, 1)], [8, 512]),                 # the smallest BIG form; the one coarse anchor is in every centre box
    'a12288': ([(96, 128)], [8]),                            # the largest BIG form
}

# (name, geometry, label generator, B, G, nc, seed).  Generators: 'centred' = the centres of the existing SimOTA test (middle 60 % of the
# canvas), 'edge' = centres from [-0.1, 1.1] * (W, H), 'far' = centred plus one row far outside the canvas on image 3 and an image (2)
# whose only row is such a one, 'many' = 200 valid rows of G = 255 clustered on a quarter of the canvas, 'corner' = centred plus, on image
# 4, a row centred just outside the canvas corner: one anchor lies in its centre box, four predictions fit it well (three of them on
# anchors that are candidates through a small neighbouring row only), so its dyn_k buys anchors whose cost carries the 1e6 term.
SIMOTA_CASES = [
    ('one-anchor', 'a1', 'centred', 24, 9, 2, 1),
    ('nine-anchors', 'a9', 'centred', 24, 9, 1, 1),
    ('three-level-centred', 'c3', 'centred', 24, 50, 2, 1),
    ('three-level-edge', 'c3', 'edge', 24, 50, 2, 1),
    ('three-level-nc100', 'c3b', 'edge', 24, 12, 100, 1),
    ('small-form-limit', 'a4096', 'centred', 24, 50, 3, 1),
    ('big-form-start', 'a4097', 'centred', 24, 50, 2, 1),
    ('big-form-limit', 'a12288', 'centred', 24, 50, 2, 1),
    ('far-rows', 'a4096', 'far', 24, 50, 2, 2),
    ('many-rows', 'a4096', 'many', 4, 255, 2, 1),
    ('corner-row', 'a4096', 'corner', 24, 50, 2, 5),
]
# what the reference must show per case (asserted without a GPU): a decided image with an anchor claimed by several rows, one with
# dyn_k >= 2.  One anchor cannot have an IoU sum of 2.
NO_DYNK2 = {'one-anchor'}


def canvas(geom):
    hws, strides = GEOMS[geom]
    return hws[0][0] * strides[0], hws[0][1] * strides[0]


def draw_simota(case):
    """float32 CPU inputs of one SimOTA case: dict(grids [A, 2], strides [A], gt_boxes, gt_cls, gt_valid, bbox, obj, cls, nc)"""
    _, geom, gen, B, G, nc, seed = case
    g = torch.Generator().manual_seed(seed)
    hws, strides = GEOMS[geom]
    H, W = canvas(geom)
    grids, svec = anchors(hws, strides, torch.float32)
    A = grids.shape[0]
    sc = min(1.0, min(H, W) / 64.0)                          # box sizes of the existing test, shrunk on the tiny canvases
    hw = torch.tensor([float(W), float(H)])
    if gen == 'many':
        n_valid = torch.full((B,), 200)
        n_valid[0] = 0
        # a quarter of the canvas; every coordinate 8 k + [1, 7], so that no centre-box edge passes within 1 of an anchor centre: with
        # 200 rows per image the in-centre margin would otherwise leave hardly an image decided
        cell = torch.randint(16, 48, (B, G, 2), generator=g).float()
        centres = cell * 8 + 1 + 6 * torch.rand(B, G, 2, generator=g)
    else:
        n_valid = torch.randint(0, min(G, 9), (B,), generator=g)
        n_valid[0] = 0
        n_valid[1] = min(G, 8)
        if gen == 'edge':
            centres = (torch.rand(B, G, 2, generator=g) * 1.2 - 0.1) * hw
        else:
            centres = torch.rand(B, G, 2, generator=g) * (hw * 0.6) + hw * 0.2
        centres[:, 1::2] = centres[:, 0::2][:, :centres[:, 1::2].shape[1]] + 6.0 * sc     # overlapping pairs -> anchors with several claimants
    gt_boxes = torch.cat([centres, (torch.rand(B, G, 2, generator=g) * 60 + 12) * sc], -1)
    gt_cls = torch.randint(0, nc, (B, G), generator=g).float()
    if gen == 'far':
        n_valid[2], n_valid[3] = 1, 4
        gt_boxes[2, 0, :2] = torch.tensor([-20.0 * W, 0.5 * H])
        gt_boxes[3, 3, :2] = torch.tensor([0.5 * W, 30.0 * H])
    for b in range(B):                                       # class ids outside [0, nc): clamped
        if b % 5 == 2 and n_valid[b] > 0:
            gt_cls[b, 0] = -1.0
        if b % 5 == 3 and n_valid[b] > 1:
            gt_cls[b, 1] = nc + 3.0
    gt_valid = torch.arange(G)[None] < n_valid[:, None]
    ctr = (grids + 0.5) * svec[:, None]
    bbox = torch.cat([ctr[None].expand(B, -1, -1) + torch.randn(B, A, 2, generator=g) * 4 * sc, (torch.rand(B, A, 2, generator=g) * 70 + 8) * sc], -1)
    obj, cls = torch.randn(B, A, generator=g) * 2, torch.randn(B, A, nc, generator=g) * 2
    if gen == 'corner':
        n_valid[4] = 3
        gt_valid = torch.arange(G)[None] < n_valid[:, None]
        gt_boxes[4, 0] = torch.tensor([-6.0, -6.0, 56.0, 56.0])
        gt_boxes[4, 1] = torch.tensor([12.0, 12.0, 20.0, 20.0])                   # a small neighbour: its centre box makes the 3 x 3 corner anchors candidates
        Wl = hws[0][1]
        for y in range(12):
            for x in range(12):
                bbox[4, y * Wl + x, 2:] = 8.0                                         # nothing else near the corner overlaps much
        for a in (0, 1, Wl, Wl + 1):
            bbox[4, a] = gt_boxes[4, 0] * torch.cat([torch.ones(2), 0.8 + 0.4 * torch.rand(2, generator=g)]) + torch.cat([torch.randn(2, generator=g) * 3, torch.zeros(2)])
    return dict(grids=grids, strides=svec, gt_boxes=gt_boxes, gt_cls=gt_cls, gt_valid=gt_valid, bbox=bbox, obj=obj, cls=cls, nc=nc)


def assign_case(d):
    """``assign`` on a draw, in float64"""
    a = to64(d['grids'], d['strides'], d['gt_boxes'], d['gt_cls'], d['gt_valid'], d['bbox'], d['obj'], d['cls'])
    return assign(*a, d['nc'])


def undecided_share(info):
    """(share of the labelled images that are undecided, number of labelled images)"""
    lab = [r for r in info if r['n'] > 0]
    return (sum(not r['decided'] for r in lab) / len(lab) if lab else 0.0), len(lab)


# the whole path (group E of the device tests, and the wrap case of group D): raw maps + labels.  (name, geometry, B, G, nc, use_l1, seed)
PATH_CASES = [
    ('three-level-l1', 'c3', 8, 50, 2, True, 1),
    ('three-level-nc3', 'c3b', 8, 12, 3, False, 1),
    ('big-form', 'a4097', 6, 50, 1, True, 1),
]
WRAP_CASE = ('loss-wrap', 'a4096', 65, 4, 1, True, 1)        # B * A = 266240 > 1024 blocks * 256 threads


def draw_path(case):
    """float32 CPU inputs of one whole-path case: raw maps per level whose decoded boxes are of the size of the labels, labels [B, G, 5]
    with image 0 empty -> dict(regs, objs, clss, labels, strides, nc, use_l1)"""
    _, geom, B, G, nc, use_l1, seed = case
    g = torch.Generator().manual_seed(seed)
    hws, strides = GEOMS[geom]
    H, W = canvas(geom)
    regs, objs, clss = [], [], []
    for (h, w), s in zip(hws, strides):
        r = torch.randn(B, 4, h, w, generator=g) * 0.4
        r[:, 2:] += math.log(28.0 / min(s, 32))
        regs.append(r)
        objs.append(torch.randn(B, 1, h, w, generator=g) * 2)
        clss.append(torch.randn(B, nc, h, w, generator=g) * 2)
    lab = torch.zeros(B, G, 5)
    for b in range(1, B):
        n = int(torch.randint(2, min(G, 6) + 1, (1,), generator=g))
        cxy = torch.rand(n, 2, generator=g) * torch.tensor([W * 0.6, H * 0.6]) + torch.tensor([W * 0.2, H * 0.2])
        cxy[1::2] = cxy[0::2][:cxy[1::2].shape[0]] + 6.0                                  # overlapping pairs -> anchors with several claimants
        lab[b, :n] = torch.cat([torch.randint(0, nc, (n, 1), generator=g).float(), cxy, torch.rand(n, 2, generator=g) * 30 + 14], 1)
    return dict(regs=regs, objs=objs, clss=clss, labels=lab, strides=strides, nc=nc, use_l1=use_l1)


def path_reference(d, need_grad=True):
    """decode -> labels -> assign -> loss in float64 on a ``draw_path`` draw -> dict(dec, gt_valid, gt_cls, gt_boxes, num_gts, fg,
    matched, matched_iou, info, values (6 tensors), grads (per level (reg, obj, cls) of d total / d raw))"""
    regs, objs, clss = to64(*d['regs']), to64(*d['objs']), to64(*d['clss'])
    lab, = to64(d['labels'])
    gt_valid, gt_cls, gt_boxes, num_gts = labels(lab)
    dec = decode(regs, objs, clss, d['strides'], sig=False)
    grids, svec = anchors([tuple(r.shape[-2:]) for r in regs], d['strides'])
    fg, matched, miou, info = assign(grids, svec, gt_boxes, gt_cls, gt_valid, dec[..., :4], dec[..., 4], dec[..., 5:], d['nc'])
    out = dict(dec=dec, gt_valid=gt_valid, gt_cls=gt_cls, gt_boxes=gt_boxes, num_gts=num_gts, fg=fg, matched=matched, matched_iou=miou,
               info=info)
    if need_grad:
        out['values'], out['grads'] = loss_and_grads(regs, objs, clss, gt_boxes, gt_cls, num_gts, fg, matched, miou, d['strides'], d['use_l1'])
    return out


def loss_and_grads(regs, objs, clss, gt_boxes, gt_cls, num_gts, fg, matched, miou, strides, use_l1):
    """``loss`` and the gradient of its total with respect to every raw map: (six detached tensors, [(g_reg, g_obj, g_cls) per level])"""
    L = len(regs)
    leaves = [t.detach().clone().requires_grad_(True) for t in list(regs) + list(objs) + list(clss)]
    vals = loss(leaves[:L], leaves[L:2 * L], leaves[2 * L:], gt_boxes, gt_cls, num_gts, fg, matched, miou, strides, use_l1)
    gr = torch.autograd.grad(vals[0], leaves)
    return [v.detach() for v in vals], [(gr[l], gr[L + l], gr[2 * L + l]) for l in range(L)]
