"""tests/detloss_ref.py without a GPU: (1) evaluated on float32-friendly inputs (every image decided) it equals
oracle.model_ref.YOLOXHead.get_assignments / get_losses -- the per-image form the goldens pin to the reference project -- and the
mirror's batch-wide YOLOXHead._assign / get_losses, both run in float32 on the CPU: assignment exact, values and gradients within float32
rounding; (2) for every seed and shape tests/test_gpu_detloss.py uses, the conditions its device comparison relies on hold on the fp64
reference alone: the share of undecided images stays within the cap, and each case still holds a decided image without labels, one with
an anchor claimed by several rows and one with dyn_k >= 2; the float32 tensor form agrees exactly on every decided image."""
import pytest
import torch

import detloss_ref as dr
import eas_snn_amd  # noqa: F401  (puts compat/ on sys.path)
from oracle import model_ref


def _decoded32(d):
    """float32 leaves and the decoded rows [B, A, 5 + nc] of a ``draw_path`` draw, built as the heads build them"""
    L = len(d['regs'])
    leaves = [t.clone().requires_grad_(True) for t in d['regs'] + d['objs'] + d['clss']]
    outs, origin, grids, svec = [], [], [], []
    for r, o, c, s in zip(leaves[:L], leaves[L:2 * L], leaves[2 * L:], d['strides']):
        H, W = r.shape[-2:]
        g, sv = dr.anchors([(H, W)], [s], torch.float32)
        out = torch.cat([r, o, c], 1).flatten(2).permute(0, 2, 1)
        outs.append(torch.cat([(out[..., :2] + g) * s, torch.exp(out[..., 2:4]) * s, out[..., 4:]], -1))
        origin.append(r.flatten(2).permute(0, 2, 1))
        grids.append(g[None])
        svec.append(sv[None])
    return leaves, torch.cat(outs, 1), origin, grids, svec


def _close(got, ref, what, rel=2e-5):
    err = float((got.detach().double() - ref).abs().max() / (1 + ref.abs().max()))
    assert err <= rel, f'{what}: {err:.3g}'


@pytest.mark.parametrize('case', dr.PATH_CASES, ids=[c[0] for c in dr.PATH_CASES])
def test_reference_equals_the_oracle_and_the_mirror(case):
    from yolox.models.yolo_head import YOLOXHead
    d = dr.draw_path(case)
    nc, L = d['nc'], len(d['regs'])
    ref = dr.path_reference(d)
    assert all(r['decided'] for r in ref['info']), 'a friendly case: every image decided'
    assert int(ref['fg'].sum()) > 0
    B, A = ref['fg'].shape
    ref_g = [g for trip in ref['grads'] for g in trip]

    # ---- the per-image original
    leaves, outputs, origin, grids, svec = _decoded32(d)
    head = model_ref.YOLOXHead(nc, width=1 / 32, strides=tuple(d['strides']), in_channels=(256,) * L)
    head.use_l1 = d['use_l1']
    xs, ys = [g[..., 0] for g in grids], [g[..., 1] for g in grids]
    vals = head.get_losses(xs, ys, svec, d['labels'], outputs, origin if d['use_l1'] else [])
    for i, (v, w) in enumerate(zip(vals, ref['values'])):
        _close(torch.as_tensor(v), w, f'oracle value {i}')
    order = [leaves[l + k * L] for l in range(L) for k in range(3)]
    for g, w in zip(torch.autograd.grad(vals[0], order), ref_g):
        _close(g, w, 'oracle gradient')
    nlabel = (d['labels'].sum(dim=2) > 0).sum(dim=1)
    with torch.no_grad():
        for b in range(B):
            n = int(nlabel[b])
            if n == 0:
                assert not ref['fg'][b].any()
                continue
            _, fg_o, iou_o, idx_o, _ = head.get_assignments(b, n, d['labels'][b, :n, 1:5], d['labels'][b, :n, 0], outputs[b, :, :4], torch.cat(svec, 1),
                                                            torch.cat(xs, 1), torch.cat(ys, 1), outputs[:, :, 5:], outputs[:, :, 4:5])
            assert torch.equal(fg_o, ref['fg'][b]) and torch.equal(idx_o, ref['matched'][b][fg_o]), f'image {b}'
            _close(iou_o, ref['matched_iou'][b][fg_o], 'oracle matched iou')

    # ---- the batch-wide mirror, tensor-op form
    leaves, outputs, origin, grids, svec = _decoded32(d)
    mirror = YOLOXHead(nc, width=1 / 32, strides=list(d['strides']), in_channels=[256] * L)
    mirror.use_l1, mirror.fused_assign, mirror.fused_loss = d['use_l1'], False, False
    vals = mirror.get_losses(torch.cat(grids, 1), torch.cat(svec, 1), d['labels'], outputs, torch.cat(origin, 1) if d['use_l1'] else None)
    for i, (v, w) in enumerate(zip(vals, ref['values'])):
        _close(torch.as_tensor(v), w, f'mirror value {i}')
    order = [leaves[l + k * L] for l in range(L) for k in range(3)]
    for g, w in zip(torch.autograd.grad(vals[0], order), ref_g):
        _close(g, w, 'mirror gradient')
    gv, gc, gb, _ = dr.labels(d['labels'])
    fg_m, m_m, iou_m = mirror._assign(torch.cat(grids, 1), torch.cat(svec, 1), gb, gc, gv, outputs[:, :, :4].detach(), outputs[:, :, 4:5].detach(),
                                      outputs[:, :, 5:].detach())
    assert torch.equal(fg_m, ref['fg']) and torch.equal(m_m[fg_m], ref['matched'][fg_m])
    _close(iou_m, ref['matched_iou'], 'mirror matched iou')


def test_labels_count_then_prefix():
    lab = torch.zeros(3, 4, 5, dtype=torch.float64)
    lab[0, 0] = torch.tensor([0.0, 5, 5, 2, 2])          # class 0 with a real box is a row
    lab[0, 2] = torch.tensor([1.0, 6, 6, 2, 2])          # behind an all-zero row: two rows counted, the first two taken
    lab[2, :3, 1:] = 1.0
    gv, gc, gb, n = dr.labels(lab)
    assert gv.tolist() == [[True, True, False, False], [False] * 4, [True, True, True, False]] and float(n) == 5.0
    assert torch.equal(gc, lab[..., 0]) and torch.equal(gb, lab[..., 1:])


@pytest.mark.parametrize('case', dr.SIMOTA_CASES, ids=[c[0] for c in dr.SIMOTA_CASES])
def test_simota_cases_keep_their_conditions(case):
    from yolox.models.yolo_head import YOLOXHead
    d = dr.draw_simota(case)
    fg, matched, miou, info = dr.assign_case(d)
    share, labelled = dr.undecided_share(info)
    assert labelled > 0 and share <= dr.CAP_UNDECIDED and share < 1.0, f'undecided share {share:.3g} of {labelled} labelled images'
    decided = [r for r in info if r['decided']]
    assert any(r['n'] == 0 for r in decided), 'no decided image without labels'
    assert any(r['multi'] > 0 for r in decided), 'no decided image with an anchor claimed by several rows'
    if case[0] not in dr.NO_DYNK2:
        assert any(max(r['dyn_k'], default=0) >= 2 for r in decided), 'no decided image with dyn_k >= 2'
    if case[2] in ('corner', 'far'):
        assert any(r['spill'] > 0 for r in info), 'no row that has to take anchors outside its own centre box'
    if case[2] == 'corner':               # decided although the row's second anchor is bought in the 1e6 range
        assert info[4]['decided'] and info[4]['spill'] > 0 and int((fg[4] & (matched[4] == 0)).sum()) >= 2
    if case[2] == 'far':
        assert info[2]['decided'] and info[2]['n'] == 1 and not info[2]['cand'].any() and not fg[2].any()
        assert info[3]['n'] == 4 and int((fg[3] & (matched[3] == 3)).sum()) <= 1
    if case[2] == 'many':
        assert all(r['n'] == 200 for r in info[1:]) and max(r['multi'] for r in info) > 100
    # the float32 tensor form on the same inputs: exact on every decided image
    head = YOLOXHead(d['nc'], width=1 / 32)
    fg_m, m_m, iou_m = head._assign(d['grids'][None], d['strides'][None], d['gt_boxes'], d['gt_cls'], d['gt_valid'], d['bbox'], d['obj'][..., None],
                                    d['cls'])
    for b, r in enumerate(info):
        if r['decided']:
            assert torch.equal(fg_m[b], fg[b]) and torch.equal(m_m[b][fg[b]], matched[b][fg[b]]), f'image {b}'
            _close(iou_m[b], miou[b], f'image {b} matched iou')


@pytest.mark.parametrize('case', dr.PATH_CASES + [dr.WRAP_CASE], ids=[c[0] for c in dr.PATH_CASES + [dr.WRAP_CASE]])
def test_path_cases_are_decided(case):
    ref = dr.path_reference(dr.draw_path(case), need_grad=False)
    bad = [(b, r['reason']) for b, r in enumerate(ref['info']) if not r['decided']]
    assert not bad, f'undecided images {bad}'
    decided = ref['info']
    assert decided[0]['n'] == 0 and int(ref['fg'].sum()) > 0
    assert any(r['multi'] > 0 for r in decided) and any(max(r['dyn_k'], default=0) >= 2 for r in decided)
