"""FocalLoss and TverskyLoss through the fused loss kernels (csrc/seg_loss.hip: ledn_focal_loss_*, ledn_tversky_loss_*,
generic and resize-folded) and their way up to LEDHead(loss_decode=[...]).

Checked, as test_seg_losses.py checks CrossEntropyLoss and DiceLoss, against (1) construction through the registry and
the rejected arguments, (2) fixtures from the reference (tests/golden/g23_*; gen_golden_focal_tversky.py says where the
Focal numbers come from), (3) the resize-folded kernels against the generic ones, against a statement-for-statement
restatement of the reference on F.interpolate(...) and against torch autograd, (4) LEDHead.loss_by_feat on the folded
and generic branches, (5) the wrappers' argument checks.  The whole training step and the CLI are in
test_focal_tversky_step.py.

Tolerances are the project's (test_seg_losses.py): kernel vs fixture loss 1e-4 / 1e-6, accuracy 1e-5 / 1e-4, gradient
1e-3 / 1e-8; folded vs restatement 2e-5 / 1e-7, folded vs generic 2e-6 / 1e-8, dsrc vs autograd 2e-4 / 1e-7; head level
losses 2e-5 / 1e-7, gradients 2e-4 / 1e-7."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import Fixture, golden_names
from oracle import spec
import test_seg_losses as TS
from test_seg_losses import CFG, ROOT, UP_CASES, D, W, close, nchw, nhwc, _up_inputs, _head_case, _Spy, ref_dice
import os

FT_CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_focal_tversky_config.py')


@pytest.fixture(autouse=True)
def _track_device(request):          # (test_seg_losses.D / nhwc follow the backend of THIS module's tests too)
    TS._DEV[0] = request.getfixturevalue('be').dev if 'be' in request.fixturenames else torch.device('cpu')
    yield


# --------------------------------------------------------------------------- #
# the reference's forwards, statement for statement (pred N x C x H x W, target N x H x W)
# --------------------------------------------------------------------------- #
def ref_focal(pred, target, use_sigmoid=True, gamma=2.0, alpha=0.5, reduction='mean', class_weight=None, loss_weight=1.0,
              ignore_index=255):
    """FocalLoss.forward's GPU branch (focal_loss.py:241-284,299-309) with the arithmetic of py_sigmoid_focal_loss
    (:45-67) and weight_reduce_loss without avg_factor (losses/utils.py:48-72).  A label outside [0, C) that is not
    ignore_index gets an all-zero row (F.one_hot(., C + 1) raises beyond C; the kernels do not)."""
    pred = pred.transpose(0, 1)
    pred = pred.reshape(pred.size(0), -1)
    pred = pred.transpose(0, 1).contiguous()
    target = target.reshape(-1).contiguous()
    valid_mask = (target != ignore_index).view(-1, 1)
    target = torch.where(target == ignore_index, target.new_tensor(0), target)
    num_classes = pred.size(1)
    target = torch.where((target < 0) | (target > num_classes), target.new_tensor(num_classes), target)
    target = F.one_hot(target, num_classes=num_classes + 1)[:, :num_classes]
    if isinstance(alpha, list):
        alpha = pred.new_tensor(alpha)
    pred_sigmoid = pred.sigmoid()
    target = target.type_as(pred)
    one_minus_pt = (1 - pred_sigmoid) * target + pred_sigmoid * (1 - target)
    focal_weight = (alpha * target + (1 - alpha) * (1 - target)) * one_minus_pt.pow(gamma)
    loss = F.binary_cross_entropy_with_logits(pred, target, reduction='none') * focal_weight
    final_weight = torch.ones(1, pred.size(1)).type_as(loss)
    if class_weight is not None:
        final_weight = final_weight * pred.new_tensor(class_weight)
    final_weight = final_weight * valid_mask
    loss = loss * final_weight
    return loss_weight * (loss.mean() if reduction == 'mean' else loss.sum())


def ref_tversky_sums(pred, target, ignore_index=255):
    """TP, FP, FN [N, C] of binary_tversky_loss (tversky_loss.py:48-54) on TverskyLoss.forward's inputs (:107-112)"""
    pred = F.softmax(pred, dim=1)
    num_classes = pred.shape[1]
    one_hot_target = F.one_hot(torch.clamp(target.long(), 0, num_classes - 1), num_classes=num_classes)
    valid_mask = (target != ignore_index).long().reshape(target.shape[0], -1)
    out = []
    for i in range(num_classes):
        p = pred[:, i].reshape(pred.shape[0], -1)
        t = one_hot_target[..., i].reshape(target.shape[0], -1)
        out.append(torch.stack([torch.sum(torch.mul(p, t) * valid_mask, dim=1),
                                torch.sum(torch.mul(p, 1 - t) * valid_mask, dim=1),
                                torch.sum(torch.mul(1 - p, t) * valid_mask, dim=1)], dim=1))
    return torch.stack(out, dim=1)          # [N, C, 3]


def ref_tversky(pred, target, smooth=1, class_weight=None, loss_weight=1.0, ignore_index=255, alpha=0.3, beta=0.7):
    """TverskyLoss.forward + tversky_loss + binary_tversky_loss, tversky_loss.py:13-57,101-123 (weighted_loss without a
    weight: the mean over the images)"""
    num_classes = pred.shape[1]
    sums = ref_tversky_sums(pred, target, ignore_index)
    total_loss = 0
    for i in range(num_classes):
        if i != ignore_index:
            TP, FP, FN = sums[:, i, 0], sums[:, i, 1], sums[:, i, 2]
            tversky = (TP + smooth) / (TP + alpha * FP + beta * FN + smooth)
            tversky_loss = (1 - tversky).mean()
            if class_weight is not None:
                tversky_loss = tversky_loss * pred.new_tensor(class_weight)[i]
            total_loss = total_loss + tversky_loss
    return loss_weight * (total_loss / num_classes)


def _ref(kind, score, tgt, kw, ignore_index=255):
    if kind == 'FocalLoss':
        return ref_focal(score, tgt, ignore_index=ignore_index, **kw)
    return ref_tversky(score, tgt, **kw)


def _kernel_kwargs(kind, kw, ignore_index):
    """fixture meta / constructor kwargs -> (family, forward kwargs, backward kwargs) of ops_train"""
    if kind == 'FocalLoss':
        a = kw.get('alpha', 0.5)
        b = dict(loss_weight=kw.get('loss_weight', 1.0), gamma=kw.get('gamma', 2.0), alpha=W(a) if isinstance(a, list) else a,
                 ignore_index=ignore_index, class_weight=W(kw.get('class_weight')), reduction=kw.get('reduction', 'mean'))
        return 'focal', b, b
    own = kw.get('ignore_index', 255)
    f = dict(loss_weight=kw.get('loss_weight', 1.0), alpha=kw.get('alpha', 0.3), beta=kw.get('beta', 0.7),
             smooth=kw.get('smooth', 1), ignore_index=own, class_weight=W(kw.get('class_weight')),
             acc_ignore_index=ignore_index)
    return 'tversky', f, dict(ignore_index=own)


# --------------------------------------------------------------------------- #
# 1. construction
# --------------------------------------------------------------------------- #
def test_losses_build_with_the_reference_defaults_and_reject_what_is_not_built():
    import led_net_amd as L
    f = L.MODELS.build(dict(type='FocalLoss'))
    assert isinstance(f, L.FocalLoss) and f.loss_name == 'loss_focal' and list(f.state_dict()) == []
    assert (f.use_sigmoid, f.gamma, f.alpha, f.reduction, f.class_weight, f.loss_weight) == \
        (True, 2.0, 0.5, 'mean', None, 1.0)
    t = L.MODELS.build(dict(type='TverskyLoss'))
    assert isinstance(t, L.TverskyLoss) and t.loss_name == 'loss_tversky' and list(t.state_dict()) == []
    assert (t.smooth, t.class_weight, t.loss_weight, t.ignore_index, t.alpha, t.beta) == (1, None, 1.0, 255, 0.3, 0.7)
    f = L.MODELS.build(dict(type='FocalLoss', gamma=1.5, alpha=[0.25, 0.6], class_weight=[0.7, 1.6], reduction='sum',
                            loss_weight=0.4, loss_name='loss_x'))
    assert f.alpha == [0.25, 0.6] and f.class_weight == [0.7, 1.6] and f.loss_name == 'loss_x'
    assert list(f.state_dict()) == []
    t = L.MODELS.build(dict(type='TverskyLoss', smooth=0.1, class_weight=[0.7, 1.6], ignore_index=0, alpha=0.5, beta=0.5,
                            loss_name='loss_y'))
    assert t.loss_name == 'loss_y' and t.ignore_index == 0 and list(t.state_dict()) == []
    for cfg, word in ((dict(type='FocalLoss', use_sigmoid=False), 'use_sigmoid'),
                      (dict(type='FocalLoss', reduction='none'), 'reduction'),
                      (dict(type='FocalLoss', class_weight='weights.npy'), 'class_weight'),
                      (dict(type='TverskyLoss', alpha=0.3, beta=0.6), 'alpha'),
                      (dict(type='TverskyLoss', class_weight='weights.npy'), 'class_weight')):
        with pytest.raises((NotImplementedError, TypeError, ValueError), match=word):
            L.MODELS.build(cfg)
    cfg = L.load_config(FT_CFG)['model']['decode_head']
    head = L.MODELS.build(cfg)
    assert [type(m).__name__ for m in head.loss_decode] == ['FocalLoss', 'TverskyLoss']
    assert head.loss_decode[0].gamma == 2.0 and head.loss_decode[1].loss_weight == 0.4 and head.loss_decode[1].beta == 0.7
    assert set(head.state_dict()) == set(L.MODELS.build(L.load_config(CFG)['model']['decode_head']).state_dict())
    for pair in (('TverskyLoss', 'FocalLoss'), ('FocalLoss', 'DiceLoss'), ('OhemCrossEntropy', 'TverskyLoss'),
                 ('CrossEntropyLoss', 'FocalLoss')):
        cfg['loss_decode'] = [dict(type=p) for p in pair]
        assert [type(m).__name__ for m in L.MODELS.build(cfg).loss_decode] == list(pair)

    class ForeignLoss(nn.Module):
        def __init__(self, loss_weight=1.0):
            super().__init__()
    L.MODELS.register_module(name='ForeignLossForTest', force=True, module=ForeignLoss)
    cfg['loss_decode'][1] = dict(type='ForeignLossForTest')
    with pytest.raises(TypeError, match='OhemCrossEntropy, CrossEntropyLoss, DiceLoss, FocalLoss, TverskyLoss'):
        L.MODELS.build(cfg)


# --------------------------------------------------------------------------- #
# 2. the reference's numbers, through the generic kernels and the modules
# --------------------------------------------------------------------------- #
GOLDEN = golden_names('g23_')


def test_golden_set_is_complete():
    assert {n[len('g23_'):] for n in GOLDEN} >= {
        'focal_default', 'focal_gamma0', 'focal_g15_a25', 'focal_alpha_list', 'focal_cw', 'focal_sum_w04', 'focal_c19',
        'focal_all_ignored', 'tversky_default', 'tversky_half_cw', 'tversky_skip_class0', 'tversky_c5', 'tversky_c19',
        'tversky_all_ignored'}


@pytest.mark.parametrize('name', GOLDEN)
def test_focal_tversky_golden(be, name):
    """the restated forward reproduces the fixture (so (3) and (4) test against the reference's arithmetic); the generic
    kernels give its loss, accuracy and gradient; so do the modules through autograd"""
    import led_net_amd as L
    from led_net_amd import ops_train as T
    fx = Fixture(name)
    kind, kw, ign = fx.meta['kind'], fx.meta['kwargs'], fx.meta['ignore_index']
    score, tgt = fx.ins['score'], fx.ins['target']
    assert 0.1 <= float((tgt == 255).float().mean()) <= 0.2 or bool((tgt == 255).all())
    torch.testing.assert_close(_ref(kind, score, tgt, kw, ign), fx.outs['loss'].reshape(()), rtol=1e-6, atol=0)
    fam, fkw, bkw = _kernel_kwargs(kind, kw, ign)
    lg, y = nhwc(score), D(tgt.contiguous())
    out, work = getattr(T, fam + '_loss_fwd')(lg, y, **fkw)
    print(name, 'loss', float(out[0]), 'want', float(fx.outs['loss']), 'acc', float(out[1]), float(fx.outs['acc']))
    close(out[0], fx.outs['loss'].reshape(()), 1e-4, 1e-6, name + ' loss')
    close(out[1], fx.outs['acc'].reshape(()), 1e-5, 1e-4, name + ' acc')
    assert float(out[2]) == 0.0 and float(out[3]) == 0.0
    dl = getattr(T, fam + '_loss_bwd')(lg, y, work, out, D(torch.ones(1)), **bkw)
    close(nchw(dl), fx.gin['score'], 1e-3, 1e-8, name + ' dscore')
    # the module, through autograd
    crit = L.MODELS.build(dict(type=kind, **kw)).to(TS._DEV[0])
    sc = nhwc(score).requires_grad_(True)
    loss = crit(sc.permute(0, 3, 1, 2), D(tgt), ignore_index=ign)
    close(loss, fx.outs['loss'].reshape(()), 1e-4, 1e-6, name + ' module loss')
    (2.0 * loss).backward()
    close(nchw(sc.grad), 2.0 * fx.gin['score'], 1e-3, 1e-8, name + ' module dscore')


def test_modules_check_list_lengths_at_call_time(be):
    import led_net_amd as L
    fx = Fixture('g23_tversky_c5')
    sc, y = nhwc(fx.ins['score']).permute(0, 3, 1, 2), D(fx.ins['target'])
    for cfg, word in ((dict(type='FocalLoss', alpha=[0.25, 0.6]), 'alpha has 2 entries'),
                      (dict(type='FocalLoss', class_weight=[1.0, 2.0]), 'class_weight has 2 entries'),
                      (dict(type='TverskyLoss', class_weight=[1.0, 2.0]), 'class_weight has 2 entries')):
        with pytest.raises(ValueError, match=word):
            L.MODELS.build(cfg).to(TS._DEV[0])(sc, y, ignore_index=255)
    with pytest.raises(ValueError, match='at most 32'):
        L.MODELS.build(dict(type='TverskyLoss')).to(TS._DEV[0])(D(torch.zeros(1, 33, 4, 4)), D(torch.zeros(1, 4, 4).long()))


def test_focal_labels_outside_the_classes_have_an_all_zero_row(be):
    """labels C, C + 7 and -3 (none of them ignore_index): every class is a negative there -- loss and gradient"""
    from led_net_amd import ops_train as T
    g = torch.Generator().manual_seed(23)
    score = (2.0 * torch.randn((1, 3, 6, 10), generator=g)).requires_grad_(True)
    tgt = torch.randint(0, 3, (1, 6, 10), generator=g)
    tgt[0, 0, :3] = torch.tensor([3, 10, -3])
    tgt[0, 1, :2] = 255
    ref = ref_focal(score, tgt, gamma=1.5, alpha=0.25)
    ref.backward()
    out, work = T.focal_loss_fwd(nhwc(score), D(tgt), gamma=1.5, alpha=0.25)
    close(out[0], ref.detach(), 2e-5, 1e-7, 'loss')
    dl = T.focal_loss_bwd(nhwc(score), D(tgt), work, out, D(torch.ones(1)), gamma=1.5, alpha=0.25)
    close(nchw(dl), score.grad, 2e-4, 1e-7, 'dscore')


# --------------------------------------------------------------------------- #
# 3. resize-folded vs generic vs the reference's statements under torch autograd
# --------------------------------------------------------------------------- #
LOSSES = [
    ('FocalLoss', dict()),
    ('FocalLoss', dict(gamma=0.0, loss_weight=0.4)),
    ('FocalLoss', dict(gamma=1.5, alpha=0.25)),
    ('FocalLoss', dict(alpha=[0.25, 0.6], class_weight=[0.7, 1.6])),
    ('FocalLoss', dict(reduction='sum', gamma=3.0)),
    ('TverskyLoss', dict()),
    ('TverskyLoss', dict(alpha=0.5, beta=0.5, smooth=0.1, class_weight=[0.7, 1.6])),
    ('TverskyLoss', dict(ignore_index=0)),
    ('TverskyLoss', dict(ignore_index=1, loss_weight=0.4)),
    ('TverskyLoss', dict(alpha=0.7, beta=0.3, smooth=1e-3)),
]


def _twice(fwd, *args, **kw):
    """`fwd` called twice -> its (out, work), after asserting that both calls gave bit-identical `out` and `work`.  The
    wrappers allocate `work` with torch.empty and the kernels write only the workgroups' part of it, so for these two
    calls the allocation is zero-filled: the WHOLE buffer is compared, with no knowledge of its layout"""
    with pytest.MonkeyPatch.context() as m:
        m.setattr(torch, 'empty', torch.zeros)
        first, second = fwd(*args, **kw), fwd(*args, **kw)
    assert torch.equal(first[0], second[0]), f'{fwd.__name__}: out differs between two calls'
    assert first[1].data_ptr() != second[1].data_ptr() and torch.equal(first[1], second[1]), \
        f'{fwd.__name__}: work differs between two calls'
    return first


@pytest.mark.parametrize('kind,kw', LOSSES, ids=[f'{k[:-4].lower()}{i}' for i, (k, _) in enumerate(LOSSES)])
@pytest.mark.parametrize('N,Hs,Ws,ignore', UP_CASES)
def test_resize_folded_vs_generic_vs_autograd(be, N, Hs, Ws, ignore, kind, kw):
    from led_net_amd import ops, ops_train as T
    s, y = _up_inputs(N, Hs, Ws, ignore)
    H, Wd = 2 * Hs, 2 * Ws
    fam, fkw, bkw = _kernel_kwargs(kind, kw, 255)
    g = torch.tensor([0.7])
    out, work = _twice(getattr(T, fam + '_loss_up_fwd'), D(s), D(y), **fkw)
    d = getattr(T, fam + '_loss_up_bwd')(D(s), D(y), work, out, D(g), **bkw).cpu()
    # the generic kernel on explicitly resized logits (the product's resize kernel)
    lg = ops.bilinear(D(s), (H, Wd))
    out2, work2 = _twice(getattr(T, fam + '_loss_fwd'), lg, D(y), **fkw)
    dl = getattr(T, fam + '_loss_bwd')(lg, D(y), work2, out2, D(g), **bkw).cpu()
    # the reference's statements on F.interpolate, gradients by autograd
    sr = s.clone().requires_grad_(True)
    up = F.interpolate(sr.permute(0, 3, 1, 2), size=(H, Wd), mode='bilinear', align_corners=False)
    ref = _ref(kind, up, y, kw)
    (ref * float(g)).backward()
    print(f'{kind} {kw}: up {float(out[0])!r} generic {float(out2[0])!r} reference {float(ref.detach())!r}')
    close(out[0], ref.detach(), 2e-5, 1e-7, 'loss: resize-folded vs reference')
    close(out2[0], ref.detach(), 2e-5, 1e-7, 'loss: generic vs reference')
    close(out[0], out2[0], 2e-6, 1e-8, 'loss: resize-folded vs generic')
    close(out[1], spec.accuracy(up.detach(), y, 255).reshape(()), 1e-5, 1e-4, 'accuracy')
    assert torch.equal(out[1], out2[1]), 'accuracy: resize-folded vs generic'
    close(d, sr.grad, 2e-4, 1e-7, 'dsrc vs autograd')
    sr2 = s.clone().requires_grad_(True)
    F.interpolate(sr2.permute(0, 3, 1, 2), size=(H, Wd), mode='bilinear', align_corners=False).backward(dl.permute(0, 3, 1, 2))
    # (the bound of test_seg_losses: the same 16 products per source pixel in two summation orders)
    close(d, sr2.grad, 1e-5, 1e-8 + 16 * 2.0 ** -24 * float(dl.abs().max()),
          'dsrc vs the generic backward pulled through the resize')
    if kind == 'TverskyLoss':         # TP, FP, FN per (image, class) in work: each image's own
        hdr, hdr2 = work[:10 * N].reshape(N, 2, 5).cpu(), work2[:10 * N].reshape(N, 2, 5).cpu()
        close(hdr[..., :3], hdr2[..., :3], 2e-6, 1e-8, 'per-(image, class) TP, FP, FN: folded vs generic')
        own = kw.get('ignore_index', 255)
        per_image = torch.cat([ref_tversky_sums(up[n:n + 1].detach(), y[n:n + 1], own) for n in range(N)])
        # sums of up to H W terms in [0, 1]: 2e-5 relative to the sum, and for the sums that nearly cancel to nothing
        # (FN of a confident class) 2^-24 per term of the largest sum of that image
        close(hdr[..., :3], per_image, 2e-5, 1e-7 + 2.0 ** -24 * float(per_image.max()), 'per-(image, class) TP, FP, FN')


def test_up_cases_cover_the_tails_and_the_row_loop():
    assert (2, 7, 9, 'border') in UP_CASES and (1, 515, 4, 'rows') in UP_CASES


# --------------------------------------------------------------------------- #
# 4. LEDHead.loss_by_feat
# --------------------------------------------------------------------------- #
_FOCAL = dict(type='FocalLoss', gamma=2.0, alpha=0.25, loss_weight=1.0)
_FOCAL_W = dict(type='FocalLoss', gamma=1.5, class_weight=[0.7, 1.6], loss_weight=0.4)
_TV = dict(type='TverskyLoss', loss_weight=0.4)
_TV_W = dict(type='TverskyLoss', alpha=0.5, beta=0.5, smooth=0.1, loss_weight=1.0)
_DICE = dict(type='DiceLoss', loss_weight=0.4)
_OHEM0 = dict(type='OhemCrossEntropy', thres=0.9, min_kept=300, loss_weight=1.0)
_OHEM1 = dict(type='OhemCrossEntropy', thres=0.8, min_kept=5000, loss_weight=0.4)
PAIRS = {'focal_tversky': (_FOCAL, _TV), 'tversky_ohem': (_TV_W, _OHEM1), 'ohem_focal': (_OHEM0, _FOCAL_W),
         'focal_dice': (_FOCAL, _DICE)}


def _ref_entry(cfg, logits, y):
    cfg = dict(cfg)
    typ = cfg.pop('type')
    if typ == 'OhemCrossEntropy':
        return spec.ohem_ce(logits, y, cfg['thres'], cfg['min_kept'], cfg['loss_weight'], 255)
    if typ == 'DiceLoss':
        return ref_dice(logits, y, **cfg)
    return _ref(typ, logits, y, cfg)


def _head_case_c(pair, hw, C):
    """test_seg_losses._head_case for C classes"""
    import led_net_amd as L
    if C == 2:
        return _head_case(pair, hw)
    H, Wd = hw
    cfg = L.load_config(CFG)['model']['decode_head']
    cfg['loss_decode'] = [dict(c) for c in pair]
    cfg['num_classes'] = C
    head = L.MODELS.build(cfg).to(TS._DEV[0]).train()
    g = torch.Generator().manual_seed(H * 100 + Wd + C)
    h8, w8 = -(-H // 8), -(-Wd // 8)
    shapes = [(2, C, h8, w8), (2, C, h8, w8), (2, C, H // 2, Wd // 2), (2, C, H // 4, Wd // 4)]     # xc, xs, h1, h2
    ref_in = [(1.5 * torch.randn(s, generator=g)).requires_grad_(True) for s in shapes]
    label = torch.randint(0, C, (2, 1, H, Wd), generator=g)
    label[:, :, :3] = 255
    ins = [nhwc(t).requires_grad_(True) for t in ref_in]
    samples = [L.SegDataSample(gt=D(label[i])) for i in range(2)]
    return head, ins, ref_in, label, samples


def _c5(cfg):
    """the pair's entry for five classes: per-class lists get five entries"""
    cfg = dict(cfg)
    if cfg.get('class_weight') is not None:
        cfg['class_weight'] = [0.5, 2.0, 1.0, 1.25, 0.8]
    return cfg


@pytest.mark.parametrize('hw,C', [((32, 40), 2), ((30, 38), 2), ((31, 37), 2), ((32, 40), 5), ((31, 37), 5)],
                         ids=['up', 'up_tail', 'generic_odd', 'c5', 'c5_odd'])
@pytest.mark.parametrize('pair', list(PAIRS))
def test_led_head_loss_by_feat_with_focal_and_tversky(be, monkeypatch, pair, hw, C):
    """LEDHead.loss_by_feat on seeded training logits vs oracle.spec.fuse_loss + the restatements: the two losses,
    acc_seg (entry 0's, whatever its type), the gradients of the four logit maps, and the entry points taken"""
    H, Wd = hw
    cfgs = PAIRS[pair] if C == 2 else tuple(_c5(c) for c in PAIRS[pair])
    head, ins, ref_in, label, samples = _head_case_c(cfgs, hw, C)
    spy = _Spy(monkeypatch)
    out = head.loss_by_feat(tuple(t.permute(0, 3, 1, 2) for t in ins), samples)
    (out['loss_context'] + 0.5 * out['loss_spatial']).backward()
    up = '_up' if H % 2 == 0 and Wd % 2 == 0 and C == 2 else ''
    fam = {'FocalLoss': f'ledn_focal_loss{up}', 'TverskyLoss': f'ledn_tversky_loss{up}', 'DiceLoss': f'ledn_dice_loss{up}',
           'OhemCrossEntropy': f'ledn_ohem_ce{up}'}
    names = [fam[c['type']] for c in cfgs]
    got = spy.take()
    assert got[:2] == [names[0] + '_fwd', names[1] + '_fwd'] and sorted(got[2:]) == sorted(n + '_bwd' for n in names), got
    xc, xs, h1, h2 = ref_in
    y = label.squeeze(1)
    ctx, spa = spec.fuse_loss(xc, h1, h2, (H, Wd)), spec.fuse_loss(xs, h1, h2, (H, Wd))
    want0, want1 = _ref_entry(cfgs[0], ctx, y), _ref_entry(cfgs[1], spa, y)
    (want0 + 0.5 * want1).backward()
    print('loss_context', float(out['loss_context']), float(want0.detach()), 'loss_spatial', float(out['loss_spatial']),
          float(want1.detach()))
    assert set(out) == {'loss_context', 'loss_spatial', 'acc_seg'}
    close(out['loss_context'].reshape(()), want0.detach(), 2e-5, 1e-7, 'loss_context')
    close(out['loss_spatial'].reshape(()), want1.detach(), 2e-5, 1e-7, 'loss_spatial')
    close(out['acc_seg'].reshape(-1), spec.accuracy(ctx.detach(), y, 255).reshape(-1), 1e-5, 1e-4, 'acc_seg')
    for name, t, r in zip(('xc', 'xs', 'h1', 'h2'), ins, ref_in):
        close(nchw(t.grad), r.grad, 2e-4, 1e-7, 'd/d' + name)


# --------------------------------------------------------------------------- #
# 5. the wrappers' argument checks
# --------------------------------------------------------------------------- #
def test_wrappers_validate_their_arguments(be):
    from led_net_amd import _lib, ops_train as T
    from led_net_amd.ops import LednError
    lg = D(torch.randn(1, 8, 8, 5))
    y5 = D(torch.randint(0, 5, (1, 8, 8)))
    s2 = D(torch.randn(1, 4, 4, 2))
    y2 = D(torch.randint(0, 2, (1, 8, 8)))
    for fwd in (T.focal_loss_fwd, T.tversky_loss_fwd):
        with pytest.raises(LednError):
            fwd(lg.double(), y5)
        with pytest.raises(LednError):
            fwd(lg, y5.int())
        with pytest.raises(LednError):
            fwd(lg, D(torch.zeros(1, 8, 9, dtype=torch.int64)))             # target of another size
        with pytest.raises(LednError):
            fwd(lg, y5, class_weight=W([1.0, 2.0]))                           # 2 weights, 5 classes
        with pytest.raises(LednError):
            fwd(lg, y5, class_weight=[1.0] * 5)                               # not a tensor
    for fwd in (T.focal_loss_up_fwd, T.tversky_loss_up_fwd):
        with pytest.raises(LednError):
            fwd(lg, y5)                                                       # five classes: no resize-folded form
        with pytest.raises(LednError):
            fwd(s2, D(torch.zeros(1, 8, 9, dtype=torch.int64)))              # not exactly twice the source
    with pytest.raises(LednError):
        T.focal_loss_fwd(lg, y5, reduction='none')
    with pytest.raises(LednError, match='alpha'):
        T.focal_loss_fwd(lg, y5, alpha=W([0.25, 0.6]))                        # 2 alphas, 5 classes
    with pytest.raises(LednError):
        T.focal_loss_fwd(lg, y5, gamma=-1.0)
    with pytest.raises(LednError, match='at most 32'):
        T.tversky_loss_fwd(D(torch.randn(1, 4, 4, 33)), D(torch.zeros(1, 4, 4, dtype=torch.int64)))
    out, work = T.tversky_loss_fwd(D(torch.randn(1, 4, 4, 32)), D(torch.zeros(1, 4, 4, dtype=torch.int64)))
    assert bool(torch.isfinite(out).all())
    out, work = T.focal_loss_up_fwd(s2, y2)
    with pytest.raises(LednError):
        T.tversky_loss_up_bwd(s2, y2, work[:4], out, D(torch.ones(1)))       # a work buffer that is not Tversky's
    # the C entry point itself refuses more than 32 classes (LEDN_EINVAL), whatever the wrapper checks
    lib = _lib.get_lib()
    assert lib.cdll.ledn_tversky_work_floats(2, 2) == 5 * 2 * 2 + 1024 * (2 + 3 * 2)
    big, yb = D(torch.randn(1, 2, 2, 33)), D(torch.zeros(1, 2, 2, dtype=torch.int64))
    wk = D(torch.zeros(lib.cdll.ledn_tversky_work_floats(1, 33)))
    rc = lib.cdll.ledn_tversky_loss_fwd(big.data_ptr(), yb.data_ptr(), 1, 4, 33, None, 0.3, 0.7, 1.0, 255, 255, 1.0,
                                        wk.data_ptr(), D(torch.zeros(4)).data_ptr(), None)
    assert rc != 0
