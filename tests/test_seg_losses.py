"""CrossEntropyLoss and DiceLoss through the fused loss kernels (csrc/seg_loss.hip: ledn_ce_loss_*, ledn_dice_loss_*,
generic and resize-folded) and their way up to LEDHead(loss_decode=[...]).

Checked against (1) construction through the registry and the rejected arguments, (2) fixtures written by the
reference's own classes (tests/golden/g22_*), (3) the resize-folded kernels against the generic ones, against a
statement-for-statement restatement of the reference's forward on F.interpolate(...) and against torch autograd,
(4) LEDHead.loss_by_feat on every dispatch branch and entry pair.  The whole training step and the CLI are in
test_seg_losses_step.py.

Tolerances are the project's: kernel vs fixture loss 1e-4 / 1e-6, gradient 1e-3 / 1e-8 (test_ops_bwd.test_ohem_golden);
head level losses 2e-5 / 1e-7, gradients 2e-4 / 1e-7, accuracy 1e-5 / 1e-4 (test_ohem_class_weight.py)."""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import Fixture, golden_names
from oracle import spec
import test_ohem_fused as TF  # (CASES and the seeded inputs of the OHEM pair test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_test_config.py')
CE_DICE_CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_ce_dice_config.py')
_DEV = [torch.device('cpu')]


@pytest.fixture(autouse=True)
def _track_device(request):
    _DEV[0] = request.getfixturevalue('be').dev if 'be' in request.fixturenames else torch.device('cpu')
    yield


def D(t):
    return t.to(_DEV[0])


def W(w):
    return None if w is None else D(torch.tensor(w, dtype=torch.float32))


def nhwc(t):
    return D(t.detach().permute(0, 2, 3, 1).contiguous())


def nchw(t):
    return t.detach().permute(0, 3, 1, 2).contiguous().cpu()


def close(a, b, rt, at, what=''):
    torch.testing.assert_close(a.detach().cpu().float(), b.detach().cpu().float(), rtol=rt, atol=at,
                               msg=lambda m: f'{what}: {m}')


# --------------------------------------------------------------------------- #
# the reference's forwards, statement for statement (pred / score N x C x H x W)
# --------------------------------------------------------------------------- #
def ref_dice(pred, target, use_sigmoid=True, activate=True, reduction='mean', naive_dice=False, loss_weight=1.0,
             ignore_index=255, eps=1e-3):
    """DiceLoss.forward + dice_loss, mmseg/models/losses/dice_loss.py:11-91,141-188"""
    num_classes = pred.shape[1]
    one_hot_target = torch.clamp(target, min=0, max=num_classes)
    one_hot_target = F.one_hot(one_hot_target, num_classes + 1)
    one_hot_target = one_hot_target[..., :num_classes].permute(0, 3, 1, 2)
    if activate:
        if use_sigmoid:
            pred = pred.sigmoid()
        elif pred.shape[1] != 1:
            pred = pred.softmax(dim=1)
    tgt = one_hot_target
    if ignore_index is not None:
        pred = pred[:, torch.arange(num_classes) != ignore_index, :, :]
        tgt = tgt[:, torch.arange(num_classes) != ignore_index, :, :]
        assert pred.shape[1] != 0
    inp = pred.flatten(1)
    tgt = tgt.flatten(1).float()
    a = torch.sum(inp * tgt, 1)
    if naive_dice:
        b = torch.sum(inp, 1)
        c = torch.sum(tgt, 1)
        d = (2 * a + eps) / (b + c + eps)
    else:
        b = torch.sum(inp * inp, 1) + eps
        c = torch.sum(tgt * tgt, 1) + eps
        d = (2 * a) / (b + c)
    loss = 1 - d
    return loss_weight * (loss.mean() if reduction == 'mean' else loss.sum())


def ref_ce(score, label, use_sigmoid=False, use_mask=False, reduction='mean', class_weight=None, loss_weight=1.0,
           avg_non_ignore=False, ignore_index=-100):
    """CrossEntropyLoss.forward + cross_entropy + weight_reduce_loss, cross_entropy_loss.py:12-78,269-296 and
    losses/utils.py:48-83.  With class weights AND ignored pixels the reference raises IndexError (class_weight[255]);
    that combination is checked against F.cross_entropy(reduction='mean') instead."""
    cw = None if class_weight is None else score.new_tensor(class_weight)
    loss = F.cross_entropy(score, label, weight=cw, reduction='none', ignore_index=ignore_index)
    avg_factor = None
    if reduction == 'mean':
        if cw is None:
            if avg_non_ignore:
                avg_factor = label.numel() - (label == ignore_index).sum().item()
            else:
                avg_factor = label.numel()
        else:
            label_weights = torch.stack([cw[cls] for cls in label.reshape(-1)]).reshape(label.shape)
            if avg_non_ignore:
                label_weights[label == ignore_index] = 0
            avg_factor = label_weights.sum()
    if avg_factor is None:
        loss = loss.sum()
    else:
        loss = loss.sum() / (avg_factor + torch.finfo(torch.float32).eps)
    return loss_weight * loss


# --------------------------------------------------------------------------- #
# 1. construction
# --------------------------------------------------------------------------- #
def test_losses_build_with_the_reference_defaults_and_reject_what_is_not_built():
    import led_net_amd as L
    d = L.MODELS.build(dict(type='DiceLoss'))
    assert isinstance(d, L.DiceLoss) and d.loss_name == 'loss_dice' and list(d.state_dict()) == []
    assert (d.use_sigmoid, d.activate, d.reduction, d.naive_dice, d.loss_weight, d.ignore_index, d.eps) == \
        (True, True, 'mean', False, 1.0, 255, 1e-3)
    c = L.MODELS.build(dict(type='CrossEntropyLoss'))
    assert isinstance(c, L.CrossEntropyLoss) and c.loss_name == 'loss_ce' and list(c.state_dict()) == []
    assert (c.use_sigmoid, c.use_mask, c.reduction, c.class_weight, c.loss_weight, c.avg_non_ignore) == \
        (False, False, 'mean', None, 1.0, False)
    c = L.MODELS.build(dict(type='CrossEntropyLoss', class_weight=[0.8, 1.2], loss_name='loss_x', avg_non_ignore=True,
                            reduction='sum', loss_weight=0.4))
    assert c.class_weight == [0.8, 1.2] and c.loss_name == 'loss_x' and list(c.state_dict()) == []
    d = L.MODELS.build(dict(type='DiceLoss', use_sigmoid=False, naive_dice=True, ignore_index=0, eps=1.0,
                            loss_name='loss_y', reduction='sum', loss_weight=3.0))
    assert d.loss_name == 'loss_y' and d.ignore_index == 0
    for cfg, word in ((dict(type='CrossEntropyLoss', use_sigmoid=True), 'use_sigmoid'),
                      (dict(type='CrossEntropyLoss', use_mask=True), 'use_mask'),
                      (dict(type='CrossEntropyLoss', reduction='none'), 'reduction'),
                      (dict(type='CrossEntropyLoss', class_weight='weights.npy'), 'class_weight'),
                      (dict(type='DiceLoss', activate=False), 'activate'),
                      (dict(type='DiceLoss', reduction='none'), 'reduction')):
        with pytest.raises((NotImplementedError, TypeError, ValueError), match=word):
            L.MODELS.build(cfg)
    # the head builds with the new losses, with a mixed pair, and names the types it supports for anything else
    cfg = L.load_config(CE_DICE_CFG)['model']['decode_head']
    head = L.MODELS.build(cfg)
    assert [type(m).__name__ for m in head.loss_decode] == ['CrossEntropyLoss', 'DiceLoss']
    assert head.loss_decode[0].avg_non_ignore is True and head.loss_decode[1].loss_weight == 0.4
    assert set(head.state_dict()) == set(L.MODELS.build(L.load_config(CFG)['model']['decode_head']).state_dict())

    class ForeignLoss(nn.Module):
        def __init__(self, loss_weight=1.0):
            super().__init__()
    L.MODELS.register_module(name='ForeignLossForTest', force=True, module=ForeignLoss)
    cfg['loss_decode'][1] = dict(type='ForeignLossForTest')
    with pytest.raises(TypeError, match='OhemCrossEntropy, CrossEntropyLoss, DiceLoss'):
        L.MODELS.build(cfg)


# --------------------------------------------------------------------------- #
# 2. the reference's own numbers, through the generic kernels
# --------------------------------------------------------------------------- #
GOLDEN = golden_names('g22_')


def test_golden_set_is_complete():
    assert {n[len('g22_'):] for n in GOLDEN} >= {
        'dice_sigmoid', 'dice_softmax', 'dice_naive', 'dice_sum_w3', 'dice_skip_class0', 'dice_c5_softmax',
        'dice_all_ignored', 'ce_plain', 'ce_ignore_avg_all', 'ce_ignore_avg_valid', 'ce_sum', 'ce_cw', 'ce_c19_cw'}


def _kernel_kwargs(kind, kw, ignore_index):
    """fixture meta -> (forward wrapper name, forward kwargs, backward kwargs) of ops_train"""
    if kind == 'DiceLoss':
        b = dict(loss_weight=kw.get('loss_weight', 1.0), use_sigmoid=kw.get('use_sigmoid', True),
                 naive_dice=kw.get('naive_dice', False), ignore_class=kw.get('ignore_index', 255),
                 eps=kw.get('eps', 1e-3), reduction=kw.get('reduction', 'mean'))
        return 'dice', dict(b, acc_ignore_index=255), b
    b = dict(loss_weight=kw.get('loss_weight', 1.0), ignore_index=ignore_index, class_weight=W(kw.get('class_weight')))
    return 'ce', dict(b, reduction=kw.get('reduction', 'mean'), avg_non_ignore=kw.get('avg_non_ignore', False)), b


@pytest.mark.parametrize('name', GOLDEN)
def test_seg_loss_golden(be, name):
    """the restated forward reproduces the fixture (so (3) and (4) test against the reference's arithmetic), and the
    generic kernels give its loss, accuracy and gradient"""
    from led_net_amd import ops_train as T
    fx = Fixture(name)
    kind, kw, ign = fx.meta['kind'], fx.meta['kwargs'], fx.meta['ignore_index']
    score, tgt = fx.ins['score'], fx.ins['target']
    ref = ref_dice(score, tgt, **kw) if kind == 'DiceLoss' else ref_ce(score, tgt, ignore_index=ign, **kw)
    torch.testing.assert_close(ref, fx.outs['loss'].reshape(()), rtol=1e-6, atol=0)
    fam, fkw, bkw = _kernel_kwargs(kind, kw, ign)
    lg, y = nhwc(score), D(tgt.contiguous())
    out, work = getattr(T, fam + '_loss_fwd')(lg, y, **fkw)
    print(name, 'loss', float(out[0]), 'want', float(fx.outs['loss']), 'acc', float(out[1]), float(fx.outs['acc']))
    close(out[0], fx.outs['loss'].reshape(()), 1e-4, 1e-6, name + ' loss')
    close(out[1], fx.outs['acc'].reshape(()), 1e-5, 1e-4, name + ' acc')
    dl = getattr(T, fam + '_loss_bwd')(lg, y, work, out, D(torch.ones(1)), **bkw)
    close(nchw(dl), fx.gin['score'], 1e-3, 1e-8, name + ' dscore')


def test_modules_forward_and_backward_match_the_fixtures(be):
    import led_net_amd as L
    for name in ('g22_dice_c5_softmax', 'g22_ce_c19_cw', 'g22_ce_ignore_avg_valid'):
        fx = Fixture(name)
        crit = L.MODELS.build(dict(type=fx.meta['kind'], **fx.meta['kwargs'])).to(_DEV[0])
        score = nhwc(fx.ins['score']).requires_grad_(True)
        loss = crit(score.permute(0, 3, 1, 2), D(fx.ins['target']), ignore_index=fx.meta['ignore_index'])
        close(loss, fx.outs['loss'].reshape(()), 1e-4, 1e-6, name + ' module loss')
        (2.0 * loss).backward()
        close(nchw(score.grad), 2.0 * fx.gin['score'], 1e-3, 1e-8, name + ' module dscore')
    wrong = L.MODELS.build(dict(type='CrossEntropyLoss', class_weight=[1.0, 2.0])).to(_DEV[0])
    fx = Fixture('g22_dice_c5_softmax')
    with pytest.raises(ValueError, match='class_weight has 2 entries'):
        wrong(nhwc(fx.ins['score']).permute(0, 3, 1, 2), D(fx.ins['target']), ignore_index=255)


def test_wrappers_validate_their_arguments(be):
    from led_net_amd import ops_train as T
    from led_net_amd.ops import LednError
    s0, _, y = TF._inputs(1, 4, 4, 'none', 3)
    lg = D(torch.randn(1, 8, 8, 5))
    y5 = D(torch.randint(0, 5, (1, 8, 8)))
    with pytest.raises(LednError):
        T.ce_loss_fwd(lg, y5, class_weight=W([1.0, 2.0]))                     # 2 weights, 5 classes
    with pytest.raises(LednError):
        T.ce_loss_fwd(lg, y5, reduction='none')
    with pytest.raises(LednError):
        T.dice_loss_fwd(lg.double(), y5)
    with pytest.raises(LednError):
        T.dice_loss_fwd(lg, y5.int())
    with pytest.raises(LednError):
        T.dice_loss_fwd(lg, D(torch.zeros(1, 8, 9, dtype=torch.int64)))      # target of another size
    with pytest.raises(LednError):
        T.ce_loss_up_fwd(D(s0), D(torch.zeros(1, 8, 9, dtype=torch.int64)))  # not exactly twice the source
    with pytest.raises(LednError):
        T.dice_loss_up_fwd(lg, y5)                                            # five classes: no resize-folded form
    with pytest.raises(LednError):
        T.ce_loss_up_fwd(D(s0), D(y), class_weight=[1.0, 2.0])                # not a tensor


# --------------------------------------------------------------------------- #
# 3. resize-folded vs generic vs the reference's statements under torch autograd
# --------------------------------------------------------------------------- #
UP_CASES = [(N, Hs, Ws, ign) for N, Hs, Ws, _, _, ign in TF.CASES] + [
    (2, 7, 9, 'border'),           # W = 18: W % 4 != 0, every row ends in a two-pixel tail
    (1, 515, 4, 'rows'),           # H = 1030 rows > the 1024 workgroups of a pass: the row loop runs twice
]
LOSSES = [
    ('dice', dict()),
    ('dice', dict(naive_dice=True, reduction='sum', loss_weight=3.0, eps=1.0)),
    ('dice', dict(use_sigmoid=False, ignore_index=1)),
    ('dice', dict(use_sigmoid=False, naive_dice=True)),
    ('ce', dict(avg_non_ignore=True)),
    ('ce', dict(avg_non_ignore=False, loss_weight=0.4)),
    ('ce', dict(reduction='sum')),
    ('ce', dict(class_weight=[0.7, 1.6], avg_non_ignore=True)),
]


def _up_inputs(N, Hs, Ws, ignore):
    """test_ohem_fused's seeded sources and ignore pattern; the labels of image n are foreground with probability
    0.1 + 0.35 n, so that per-image sums that leak into a neighbour show"""
    s0, _, y = TF._inputs(N, Hs, Ws, ignore, 7 + N)
    g = torch.Generator().manual_seed(100 + N)
    fg = torch.stack([(torch.rand(y.shape[1:], generator=g) < 0.1 + 0.35 * n).long() for n in range(N)])
    return s0, torch.where(y == 255, y, fg)


@pytest.mark.parametrize('fam,kw', LOSSES, ids=[f'{f}{i}' for i, (f, _) in enumerate(LOSSES)])
@pytest.mark.parametrize('N,Hs,Ws,ignore', UP_CASES)
def test_resize_folded_vs_generic_vs_autograd(be, N, Hs, Ws, ignore, fam, kw):
    from led_net_amd import ops, ops_train as T
    s, y = _up_inputs(N, Hs, Ws, ignore)
    H, Wd = 2 * Hs, 2 * Ws
    kind = 'DiceLoss' if fam == 'dice' else 'CrossEntropyLoss'
    _, fkw, bkw = _kernel_kwargs(kind, kw, 255)
    g = torch.tensor([0.7])
    out, work = getattr(T, fam + '_loss_up_fwd')(D(s), D(y), **fkw)
    d = getattr(T, fam + '_loss_up_bwd')(D(s), D(y), work, out, D(g), **bkw).cpu()
    # the generic kernel on explicitly resized logits (the product's resize kernel)
    lg = ops.bilinear(D(s), (H, Wd))
    out2, work2 = getattr(T, fam + '_loss_fwd')(lg, D(y), **fkw)
    dl = getattr(T, fam + '_loss_bwd')(lg, D(y), work2, out2, D(g), **bkw).cpu()
    # the reference's statements on F.interpolate, gradients by autograd
    sr = s.clone().requires_grad_(True)
    up = F.interpolate(sr.permute(0, 3, 1, 2), size=(H, Wd), mode='bilinear', align_corners=False)
    if fam == 'dice':
        ref = ref_dice(up, y, **kw)
    elif kw.get('class_weight') is not None and bool((y == 255).any()):
        assert kw.get('reduction', 'mean') == 'mean'
        ref = kw.get('loss_weight', 1.0) * F.cross_entropy(up, y, weight=torch.tensor(kw['class_weight']), ignore_index=255,
                                                         reduction='mean')
        if ignore == 'all':
            ref = up.sum() * 0.0          # (F.cross_entropy: 0 / 0; the kernels and the unweighted reference give 0)
    else:
        ref = ref_ce(up, y, ignore_index=255, **kw)
    (ref * float(g)).backward()
    print(f'{fam} {kw}: up {float(out[0])!r} generic {float(out2[0])!r} reference {float(ref.detach())!r}')
    close(out[0], ref.detach(), 2e-5, 1e-7, 'loss: resize-folded vs reference')
    close(out2[0], ref.detach(), 2e-5, 1e-7, 'loss: generic vs reference')
    close(out[0], out2[0], 2e-6, 1e-8, 'loss: resize-folded vs generic')
    close(out[1], spec.accuracy(up.detach(), y, 255).reshape(()), 1e-5, 1e-4, 'accuracy')
    close(out[1], out2[1], 0, 0, 'accuracy: resize-folded vs generic')
    if fam == 'ce':
        assert float(out[3]) == float((y != 255).sum()) == float(out2[3])
    close(d, sr.grad, 2e-4, 1e-7, 'dsrc vs autograd')
    sr2 = s.clone().requires_grad_(True)
    F.interpolate(sr2.permute(0, 3, 1, 2), size=(H, Wd), mode='bilinear', align_corners=False).backward(dl.permute(0, 3, 1, 2))
    # the same 16 products per source pixel in two summation orders: each order rounds at most 16 times at the size of
    # the largest product (<= max |dlogits|), which bounds the absolute difference where the products cancel
    # (reduction='sum' has gradients of order 1, where a fixed 1e-8 is a quarter of an ulp of one product)
    close(d, sr2.grad, 1e-5, 1e-8 + 16 * 2.0 ** -24 * float(dl.abs().max()),
          'dsrc vs the generic backward pulled through the resize')
    if fam == 'dice':         # the per-image sums a, b, c in work: each image's own
        hdr, hdr2 = work[:4 * N].reshape(N, 4).cpu(), work2[:4 * N].reshape(N, 4).cpu()
        close(hdr, hdr2, 2e-6, 1e-8, 'per-image a, b, c, loss_n')
        per_image = torch.stack([ref_dice(up[n:n + 1].detach(), y[n:n + 1], **dict(kw, reduction='sum', loss_weight=1.0))
                                 for n in range(N)])
        close(hdr[:, 3], per_image, 2e-5, 1e-7, 'per-image loss_n')


# --------------------------------------------------------------------------- #
# 4. LEDHead.loss_by_feat
# --------------------------------------------------------------------------- #
_CE = dict(type='CrossEntropyLoss', avg_non_ignore=True, loss_weight=1.0)
_CEW = dict(type='CrossEntropyLoss', class_weight=[0.7, 1.6], loss_weight=0.4)
_DICE = dict(type='DiceLoss', loss_weight=0.4)
_DICE_SM = dict(type='DiceLoss', use_sigmoid=False, naive_dice=True, loss_weight=1.0)
_OHEM0 = dict(type='OhemCrossEntropy', thres=0.9, min_kept=300, loss_weight=1.0)
_OHEM1 = dict(type='OhemCrossEntropy', thres=0.8, min_kept=5000, loss_weight=0.4)
PAIRS = {'ce_dice': (_CE, _DICE), 'dice_ohem': (_DICE_SM, _OHEM1), 'ohem_ce': (_OHEM0, _CEW), 'dice_dice': (_DICE, _DICE_SM)}


def _ref_entry(cfg, logits, y):
    cfg = dict(cfg)
    typ = cfg.pop('type')
    if typ == 'OhemCrossEntropy':
        return spec.ohem_ce(logits, y, cfg['thres'], cfg['min_kept'], cfg['loss_weight'], 255)
    if typ == 'DiceLoss':
        return ref_dice(logits, y, **cfg)
    if cfg.get('class_weight') is not None:          # weights and ignored pixels: the reference raises (see ref_ce)
        return cfg['loss_weight'] * F.cross_entropy(logits, y, weight=torch.tensor(cfg['class_weight']), ignore_index=255,
                                                    reduction='mean')
    return ref_ce(logits, y, ignore_index=255, **cfg)


class _Spy:
    def __init__(self, monkeypatch):
        from led_net_amd import _lib
        self.names = []
        orig = _lib.Library.call

        def call(lib, name, *args):
            self.names.append(name)
            return orig(lib, name, *args)
        monkeypatch.setattr(_lib.Library, 'call', call)

    def take(self):
        n, self.names = [x for x in self.names if 'ohem' in x or '_loss_' in x], []
        return n


def _head_case(pair, hw, seed_extra=0):
    import led_net_amd as L
    H, Wd = hw
    cfg = L.load_config(CFG)['model']['decode_head']
    cfg['loss_decode'] = [dict(c) for c in pair]
    head = L.MODELS.build(cfg).to(_DEV[0]).train()
    g = torch.Generator().manual_seed(H * 100 + Wd + seed_extra)
    h8, w8 = -(-H // 8), -(-Wd // 8)
    shapes = [(2, 2, h8, w8), (2, 2, h8, w8), (2, 2, H // 2, Wd // 2), (2, 2, H // 4, Wd // 4)]     # xc, xs, h1, h2
    ref_in = [(1.5 * torch.randn(s, generator=g)).requires_grad_(True) for s in shapes]
    label = torch.stack([(torch.rand((1, H, Wd), generator=g) < 0.15 + 0.5 * n).long() for n in range(2)])
    label[:, :, :3] = 255
    ins = [nhwc(t).requires_grad_(True) for t in ref_in]
    samples = [L.SegDataSample(gt=D(label[i])) for i in range(2)]
    return head, ins, ref_in, label, samples


@pytest.mark.parametrize('hw', [(32, 40), (30, 38), (31, 37)], ids=['up', 'up_tail', 'generic'])
@pytest.mark.parametrize('pair', list(PAIRS))
def test_led_head_loss_by_feat_with_the_new_losses(be, monkeypatch, pair, hw):
    """LEDHead.loss_by_feat on seeded training logits vs oracle.spec.fuse_loss + the reference's statements: the two
    losses, acc_seg (entry 0's, whatever its type) and the gradients of the four logit maps; and the entry points
    taken on this branch"""
    H, Wd = hw
    head, ins, ref_in, label, samples = _head_case(PAIRS[pair], hw)
    spy = _Spy(monkeypatch)
    out = head.loss_by_feat(tuple(t.permute(0, 3, 1, 2) for t in ins), samples)
    (out['loss_context'] + 0.5 * out['loss_spatial']).backward()
    up = '_up' if H % 2 == 0 and Wd % 2 == 0 else ''
    fam = {'CrossEntropyLoss': f'ledn_ce_loss{up}', 'DiceLoss': f'ledn_dice_loss{up}', 'OhemCrossEntropy': f'ledn_ohem_ce{up}'}
    names = [fam[c['type']] + ('_w' if c['type'] == 'OhemCrossEntropy' and c.get('class_weight') else '') for c in PAIRS[pair]]
    got = spy.take()
    assert got[:2] == [names[0] + '_fwd', names[1] + '_fwd'] and sorted(got[2:]) == sorted(n + '_bwd' for n in names), got
    xc, xs, h1, h2 = ref_in
    y = label.squeeze(1)
    ctx, spa = spec.fuse_loss(xc, h1, h2, (H, Wd)), spec.fuse_loss(xs, h1, h2, (H, Wd))
    want0, want1 = _ref_entry(PAIRS[pair][0], ctx, y), _ref_entry(PAIRS[pair][1], spa, y)
    (want0 + 0.5 * want1).backward()
    print('loss_context', float(out['loss_context']), float(want0.detach()), 'loss_spatial', float(out['loss_spatial']),
          float(want1.detach()))
    assert set(out) == {'loss_context', 'loss_spatial', 'acc_seg'}
    close(out['loss_context'].reshape(()), want0.detach(), 2e-5, 1e-7, 'loss_context')
    close(out['loss_spatial'].reshape(()), want1.detach(), 2e-5, 1e-7, 'loss_spatial')
    close(out['acc_seg'].reshape(-1), spec.accuracy(ctx.detach(), y, 255).reshape(-1), 1e-5, 1e-4, 'acc_seg')
    for name, t, r in zip(('xc', 'xs', 'h1', 'h2'), ins, ref_in):
        close(nchw(t.grad), r.grad, 2e-4, 1e-7, 'd/d' + name)


def test_two_ohem_entries_keep_their_launches(be, monkeypatch):
    """[OhemCrossEntropy, OhemCrossEntropy] (the default config) issues exactly the pair's entry points, on every
    branch what it issued before the new losses existed, and none of theirs"""
    want = {(32, 40): ['ledn_ohem2_up_fwd', 'ledn_ohem2_up_bwd'],
            (30, 38): ['ledn_ohem_ce_up_fwd', 'ledn_ohem_ce_up_fwd', 'ledn_ohem_ce_up_bwd', 'ledn_ohem_ce_up_bwd'],
            (31, 37): ['ledn_ohem_ce_fwd', 'ledn_ohem_ce_fwd', 'ledn_ohem_ce_bwd', 'ledn_ohem_ce_bwd']}
    for hw, names in want.items():
        head, ins, _, _, samples = _head_case((_OHEM0, _OHEM1), hw)
        spy = _Spy(monkeypatch)
        out = head.loss_by_feat(tuple(t.permute(0, 3, 1, 2) for t in ins), samples)
        (out['loss_context'] + out['loss_spatial']).backward()
        got = spy.take()
        assert got == names and not any('_loss_' in n for n in got), (hw, got)
        monkeypatch.undo()
