"""LovaszLoss through csrc/lovasz.hip (an on-device radix sort of the per-class errors and the closed-form Lovasz gradient)
and its way up to LEDHead(loss_decode=[...]).

Checked against (1) construction through the registry and the rejected arguments, (2) fixtures from the reference
(tests/golden/g24_lovasz_*; gen_golden_lovasz.py), (3) a statement-for-statement restatement of the reference on f64
tensors under torch autograd, on inputs whose errors are well separated, (4) inputs FULL of ties, where only
order-independent properties are asserted, (5) LEDHead.loss_by_feat, (6) the wrappers' argument checks.  The whole
training step and the CLI are in test_lovasz_step.py.

Tolerances.  Loss 1e-4 / 1e-6 and accuracy 1e-5 / 1e-4 are the project's (test_seg_losses.py).  Gradient against the
f64 restatement: the project's 1e-3 / 1e-8.  Gradient against the REFERENCE's f32 fixtures: rtol 1e-3 and
atol = 2e-7 * loss_weight -- the reference forms the Lovasz gradient g as the f32 difference J_i - J_(i-1) of two
Jaccard values of size ~1, which carries about 1.2e-7 absolute rounding whatever the size of g (1 / U); d error /
d logit = p (1 - p) <= 1/4 scales it, and a factor of a few covers the sum over the classes and the softmax row:
1.2e-7 * 1/4 * ~6 = 2e-7, times loss_weight.  The kernels form g in closed form from integer counts and do not have
that error (the f64 cases hold them to 1e-8)."""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import Fixture, golden_names
import test_seg_losses as TS
from test_seg_losses import CFG, ROOT, D, W, close, nchw, nhwc, _Spy

LV_CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_lovasz_config.py')


@pytest.fixture(autouse=True)
def _track_device(request):          # (test_seg_losses.D / nhwc follow the backend of THIS module's tests too)
    TS._DEV[0] = request.getfixturevalue('be').dev if 'be' in request.fixturenames else torch.device('cpu')
    yield


# --------------------------------------------------------------------------- #
# the reference's forward, statement for statement, in the dtype of `pred` (lovasz_loss.py:15-27,43-57,129-222,280-309)
# --------------------------------------------------------------------------- #
def ref_lovasz_grad(gt_sorted):
    p = len(gt_sorted)
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1 - gt_sorted).cumsum(0)
    jaccard = 1. - intersection / union
    if p > 1:
        jaccard[1:p] = jaccard[1:p] - jaccard[0:-1]
    return jaccard


def ref_flatten_probs(probs, labels, ignore_index):
    B, C, H, Wd = probs.size()
    probs = probs.permute(0, 2, 3, 1).contiguous().view(-1, C)
    labels = labels.view(-1)
    valid = (labels != ignore_index)
    return probs[valid.nonzero().reshape(-1)], labels[valid]


def ref_lovasz_flat(probs, labels, classes, class_weight):
    if probs.numel() == 0:
        return probs.sum() * 0.          # (the reference returns an empty tensor here; the kernels' 0)
    C = probs.size(1)
    losses = []
    class_to_sum = list(range(C)) if classes in ['all', 'present'] else classes
    for c in class_to_sum:
        fg = (labels == c).to(probs.dtype)
        if classes == 'present' and fg.sum() == 0:
            continue
        errors = (fg - probs[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        fg_sorted = fg[perm.data]
        loss = torch.dot(errors_sorted, ref_lovasz_grad(fg_sorted))
        if class_weight is not None:
            loss = loss * class_weight[c]
        losses.append(loss)
    if not losses:
        return probs.sum() * 0.
    return torch.stack(losses).mean()


def ref_lovasz(pred, target, loss_type='multi_class', classes='present', per_image=False, reduction='mean',
               class_weight=None, loss_weight=1.0, ignore_index=255, probs=None):
    """LovaszLoss.forward; probs: class probabilities to use instead of softmax(pred) (the ties tests hand in the
    f32-rounded ones)"""
    cw = None if class_weight is None else pred.new_tensor(class_weight)
    probs = F.softmax(pred, dim=1) if probs is None else probs
    if per_image:
        loss = torch.stack([ref_lovasz_flat(*ref_flatten_probs(p.unsqueeze(0), l.unsqueeze(0), ignore_index), classes, cw)
                            for p, l in zip(probs, target)])
        loss = loss.mean() if reduction == 'mean' else loss.sum()
    else:
        loss = ref_lovasz_flat(*ref_flatten_probs(probs, target, ignore_index), classes, cw)
    return loss_weight * loss


def _fwd_kwargs(kw, ignore_index=255):
    red = kw.get('reduction', 'mean')
    return dict(loss_weight=kw.get('loss_weight', 1.0), classes=kw.get('classes', 'present'),
                per_image=kw.get('per_image', False), reduction='mean' if red == 'none' else red,
                ignore_index=ignore_index, class_weight=W(kw.get('class_weight')))


def _run_kernels(score, tgt, kw, dloss=1.0):
    """ops_train forward + backward on NCHW `score` -> (out, work, d score NCHW on the CPU)"""
    from led_net_amd import ops_train as T
    lg, y = nhwc(score), D(tgt.contiguous())
    out, work = T.lovasz_loss_fwd(lg, y, **_fwd_kwargs(kw))
    dl = T.lovasz_loss_bwd(lg, y, work, out, D(torch.tensor([dloss])))
    return out, work, nchw(dl)


# --------------------------------------------------------------------------- #
# 1. construction
# --------------------------------------------------------------------------- #
def test_lovasz_builds_with_the_reference_defaults_and_rejects_what_is_not_built():
    import led_net_amd as L
    with pytest.raises(ValueError, match="mmseg requires reduction='none'"):
        L.MODELS.build(dict(type='LovaszLoss'))          # (the reference's own defaults fail its assert, :269-271)
    m = L.MODELS.build(dict(type='LovaszLoss', reduction='none'))
    assert isinstance(m, L.LovaszLoss) and m.loss_name == 'loss_lovasz' and list(m.state_dict()) == []
    assert (m.loss_type, m.classes, m.per_image, m.reduction, m.class_weight, m.loss_weight) == \
        ('multi_class', 'present', False, 'none', None, 1.0)
    m = L.MODELS.build(dict(type='LovaszLoss', classes=[1, 0], per_image=True, reduction='sum', class_weight=[0.7, 1.6],
                            loss_weight=0.4, loss_name='loss_x'))
    assert (m.classes, m.per_image, m.reduction, m.class_weight, m.loss_name) == ([1, 0], True, 'sum', [0.7, 1.6], 'loss_x')
    assert list(m.state_dict()) == []
    assert L.MODELS.build(dict(type='LovaszLoss', per_image=True)).reduction == 'mean'
    for cfg, exc, word in (
            (dict(type='LovaszLoss', loss_type='binary', reduction='none'), NotImplementedError, 'loss_type'),
            (dict(type='LovaszLoss', loss_type='hinge', reduction='none'), ValueError, 'loss_type'),
            (dict(type='LovaszLoss', per_image=True, reduction='none'), NotImplementedError, 'reduction'),
            (dict(type='LovaszLoss', per_image=True, reduction='max'), ValueError, 'reduction'),
            (dict(type='LovaszLoss', reduction='mean'), ValueError, 'reduction'),
            (dict(type='LovaszLoss', reduction='sum'), ValueError, "mmseg requires reduction='none'"),
            (dict(type='LovaszLoss', reduction='none', class_weight='weights.npy'), TypeError, 'class_weight'),
            (dict(type='LovaszLoss', reduction='none', class_weight=[]), ValueError, 'class_weight'),
            (dict(type='LovaszLoss', reduction='none', classes='some'), ValueError, 'classes'),
            (dict(type='LovaszLoss', reduction='none', classes=[]), ValueError, 'classes'),
            (dict(type='LovaszLoss', reduction='none', classes=[0, 0]), ValueError, 'classes'),
            (dict(type='LovaszLoss', reduction='none', classes=[0.5]), ValueError, 'classes'),
            (dict(type='LovaszLoss', reduction='none', classes=[-1]), ValueError, 'classes')):
        with pytest.raises(exc, match=word):
            L.MODELS.build(cfg)
    cfg = L.load_config(LV_CFG)['model']['decode_head']
    head = L.MODELS.build(cfg)
    assert [type(m).__name__ for m in head.loss_decode] == ['CrossEntropyLoss', 'LovaszLoss']
    assert head.loss_decode[1].loss_weight == 0.4 and head.loss_decode[1].reduction == 'none'
    assert set(head.state_dict()) == set(L.MODELS.build(L.load_config(CFG)['model']['decode_head']).state_dict())
    lv = dict(type='LovaszLoss', reduction='none')
    for pair in ((lv, dict(type='DiceLoss')), (dict(type='OhemCrossEntropy'), lv), (lv, lv), (dict(type='FocalLoss'), lv)):
        cfg['loss_decode'] = [dict(p) for p in pair]
        assert [type(m).__name__ for m in L.MODELS.build(cfg).loss_decode] == [p['type'] for p in pair]

    class ForeignLoss(nn.Module):
        def __init__(self, loss_weight=1.0):
            super().__init__()
    L.MODELS.register_module(name='ForeignLossForLovaszTest', force=True, module=ForeignLoss)
    cfg['loss_decode'][1] = dict(type='ForeignLossForLovaszTest')
    with pytest.raises(TypeError, match='OhemCrossEntropy, CrossEntropyLoss, DiceLoss, FocalLoss, TverskyLoss, LovaszLoss$'):
        L.MODELS.build(cfg)


# --------------------------------------------------------------------------- #
# 2. the reference's numbers
# --------------------------------------------------------------------------- #
GOLDEN = golden_names('g24_lovasz_')


def test_golden_set_is_complete():
    assert {n[len('g24_lovasz_'):] for n in GOLDEN} >= {
        'default', 'all', 'list1', 'cw', 'per_image_mean', 'per_image_sum', 'c5', 'c19_few', 'c19_all', 'ignore12',
        'no_class1'}
    for n in GOLDEN:
        assert Fixture(n).ins['target'].numel() <= 8192


@pytest.mark.parametrize('name', GOLDEN)
def test_lovasz_golden(be, name):
    """the restated forward (f32) reproduces the fixture; the kernels give its loss, accuracy and gradient; so does the
    module through autograd"""
    import led_net_amd as L
    fx = Fixture(name)
    kw, ign = fx.meta['kwargs'], fx.meta['ignore_index']
    score, tgt = fx.ins['score'], fx.ins['target']
    assert ign == 255 and 0.05 <= float((tgt == 255).float().mean()) <= 0.2
    if name.endswith('ignore12'):
        assert 0.11 <= float((tgt == 255).float().mean()) <= 0.13
    if name.endswith('no_class1'):
        assert not bool((tgt[1] == 1).any()) and bool((tgt[0] == 1).any())
    if 'c19' in name:
        assert len(set(tgt[tgt != 255].tolist())) == 5
    torch.testing.assert_close(ref_lovasz(score, tgt, **kw), fx.outs['loss'].reshape(()), rtol=1e-6, atol=0)
    lw = kw.get('loss_weight', 1.0)
    out, work, dscore = _run_kernels(score, tgt, kw)
    print(name, 'loss', float(out[0]), 'want', float(fx.outs['loss']), 'acc', float(out[1]), float(fx.outs['acc']),
          'max |d| err', float((dscore - fx.gin['score']).abs().max()), 'max |d|', float(fx.gin['score'].abs().max()))
    close(out[0], fx.outs['loss'].reshape(()), 1e-4, 1e-6, name + ' loss')
    close(out[1], fx.outs['acc'].reshape(()), 1e-5, 1e-4, name + ' acc')
    assert float(out[3]) == float((tgt != 255).sum())
    close(dscore, fx.gin['score'], 1e-3, 2e-7 * lw, name + ' dscore')
    crit = L.MODELS.build(dict(type='LovaszLoss', **kw)).to(TS._DEV[0])
    sc = nhwc(score).requires_grad_(True)
    loss = crit(sc.permute(0, 3, 1, 2), D(tgt), ignore_index=ign)
    close(loss, fx.outs['loss'].reshape(()), 1e-4, 1e-6, name + ' module loss')
    (2.0 * loss).backward()
    close(nchw(sc.grad), 2.0 * fx.gin['score'], 1e-3, 4e-7 * lw, name + ' module dscore')


# --------------------------------------------------------------------------- #
# 3. against the f64 restatement under autograd, errors well separated
# --------------------------------------------------------------------------- #
def _labels(N, C, H, Wd, g, present=None, ignore=True):
    if present is None:
        y = torch.randint(0, C, (N, H, Wd), generator=g)
    else:
        y = torch.tensor(present)[torch.randint(0, len(present), (N, H, Wd), generator=g)]
    if ignore:
        y[torch.rand((N, H, Wd), generator=g) < 0.1] = 255
        y[:, :2, :] = 255
    return y


def gridded_case(N, H, Wd, seed, ignore=True):
    """two classes: the errors are a random permutation of the grid (k + 0.5) / P, P = N H W (spaced 1 / P), p_1 = the
    probability with that error for the pixel's label, x_1 - x_0 = logit(p_1)"""
    g = torch.Generator().manual_seed(seed)
    P = N * H * Wd
    y = _labels(N, 2, H, Wd, g, ignore=ignore)
    e = ((torch.randperm(P, generator=g).double() + 0.5) / P).reshape(N, H, Wd)
    p1 = torch.where(y == 1, 1.0 - e, e)
    half = 0.5 * (torch.log(p1) - torch.log1p(-p1))
    return torch.stack([-half, half], dim=1).float(), y


def separated_case(N, C, H, Wd, seed, present=None, scale=2.0, gap=2e-6):
    """C > 2: seeded logits; every pixel whose error in some class lies within `gap` of another valid pixel's (of the
    batch) is drawn again until none does"""
    g = torch.Generator().manual_seed(seed)
    y = _labels(N, C, H, Wd, g, present)
    x = scale * torch.randn((N, C, H, Wd), generator=g)
    for _ in range(500):
        bad = _close_pixels(x, y, gap)
        if not bool(bad.any()):
            return x, y
        x.permute(0, 2, 3, 1)[bad] = scale * torch.randn((int(bad.sum()), C), generator=g)
    raise AssertionError('no separated draw found')


def _close_pixels(x, y, gap):
    p = torch.softmax(x.double(), dim=1)
    valid = y != 255
    bad = torch.zeros_like(valid)
    for c in range(x.shape[1]):
        e = ((y == c).double() - p[:, c]).abs()[valid]
        es, order = torch.sort(e)
        near = (es[1:] - es[:-1]) < gap
        flag = torch.zeros_like(es, dtype=torch.bool)
        flag[1:] |= near          # (one pixel of a close pair: drawing both again makes new pairs as fast as it removes them)
        t = torch.zeros_like(valid)
        hit = torch.zeros_like(flag)
        hit[order] = flag
        t[valid] = hit
        bad |= t
    return bad


def _min_gap(x, y):
    """the smallest distance between two valid pixels' errors of one class, in f64 on the f32 logits"""
    p = torch.softmax(x.double(), dim=1)
    valid = y != 255
    gaps = []
    for c in range(x.shape[1]):
        es = torch.sort(((y == c).double() - p[:, c]).abs()[valid])[0]
        gaps.append(float((es[1:] - es[:-1]).min()))
    return min(gaps)


def _check_f64(x, y, kw, dev=None):
    """kernels on f32 x against the restatement on x.double() (on `dev`) with autograd"""
    xd = x.double().to(dev or 'cpu').requires_grad_(True)
    want = ref_lovasz(xd, y.to(xd.device), **kw)
    want.backward()
    out, work, dscore = _run_kernels(x, y, kw)
    gw = xd.grad.cpu()
    print(kw, tuple(x.shape), 'loss', float(out[0]), float(want.detach()), 'max |d| err', float((dscore - gw).abs().max()),
          'max |d|', float(gw.abs().max()))
    close(out[0], want.detach(), 1e-4, 1e-6, 'loss')
    torch.testing.assert_close(dscore.double(), gw, rtol=1e-3, atol=1e-8, msg=lambda m: f'dscore {kw}: {m}')
    return out, work


def test_shapes_cover_the_tile_paths():
    from led_net_amd.ops_train import LOVASZ_TILE
    assert 2 * 24 * 20 < LOVASZ_TILE                                  # less than one tile
    assert 37 * 53 < LOVASZ_TILE < 2 * 37 * 53 and (2 * 37 * 53) % LOVASZ_TILE      # per image one tile, batch: a partial second
    for n in (127 * 161, 2 * 127 * 161):                              # cross-workgroup digit offsets, cross-tile scan
        assert n >= 3 * LOVASZ_TILE and n % LOVASZ_TILE != 0


@pytest.mark.parametrize('kw', [dict(reduction='none'), dict(classes='all', reduction='none', loss_weight=0.4),
                                dict(per_image=True), dict(per_image=True, reduction='sum', class_weight=[0.7, 1.6])],
                         ids=['default', 'all', 'per_image', 'per_image_sum_cw'])
def test_lovasz_vs_f64_less_than_one_tile(be, kw):
    x, y = gridded_case(2, 24, 20, 1)
    assert _min_gap(x, y) > 0.5 / (2 * 24 * 20)
    _check_f64(x, y, kw)


@pytest.mark.parametrize('per_image', [False, True])
def test_lovasz_vs_f64_odd_sizes_three_classes(be, per_image):
    """2 x 3 x 37 x 53: a partial last tile, ignored pixels, class 2 absent from image 1"""
    x, y = separated_case(2, 3, 37, 53, 2)
    y[1][y[1] == 2] = 0
    x, y = _separate_again(x, y)
    assert _min_gap(x, y) >= 2e-6 and not bool((y[1] == 2).any()) and bool((y[0] == 2).any())
    kw = dict(per_image=True, class_weight=[0.5, 2.0, 1.25]) if per_image else dict(reduction='none', class_weight=[0.5, 2.0, 1.25])
    out, _ = _check_f64(x, y, kw)
    assert float(out[2]) == (2.0 if per_image else 3.0) and float(out[3]) == float((y != 255).sum())


def _separate_again(x, y, gap=2e-6, scale=2.0):
    g = torch.Generator().manual_seed(99)
    for _ in range(500):
        bad = _close_pixels(x, y, gap)
        if not bool(bad.any()):
            return x, y
        x.permute(0, 2, 3, 1)[bad] = scale * torch.randn((int(bad.sum()), x.shape[1]), generator=g)
    raise AssertionError('no separated draw found')


@pytest.mark.parametrize('classes', ['present', 'all', [3, 18, 5]], ids=['present', 'all', 'list'])
def test_lovasz_vs_f64_nineteen_classes_five_present(be, classes):
    """1 x 19 x 32 x 48, labels from five classes; the list holds two present classes and an absent one (whose loss is
    the largest error: lovasz_grad with G = 0)"""
    # (logit scale 1: with 19 classes, wider logits crowd the small probabilities of the 18 background classes below
    # 1e-3, where 1 500 pixels cannot keep 2e-6 apart)
    x, y = separated_case(1, 19, 32, 48, 3, present=[0, 3, 7, 11, 18], scale=1.0)
    assert _min_gap(x, y) >= 2e-6
    out, _ = _check_f64(x, y, dict(classes=classes, reduction='none'))
    assert float(out[2]) == {'present': 5.0, 'all': 19.0}.get(classes if isinstance(classes, str) else '', 3.0)


@pytest.mark.parametrize('per_image', [False, True])
def test_lovasz_vs_f64_many_tiles(be, per_image):
    """2 x 2 x 127 x 161, gridded: at least three tiles per segment and a partial last one, batch-wide and per image"""
    x, y = gridded_case(2, 127, 161, 4)
    assert _min_gap(x, y) > 0.5 / (2 * 127 * 161)
    _check_f64(x, y, dict(per_image=True) if per_image else dict(reduction='none'))


@pytest.mark.gpu
def test_lovasz_vs_f64_hundreds_of_workgroups():
    """1 x 2 x 512 x 512, gridded: 128 workgroups in every pass, against the f64 restatement run on the device"""
    TS._DEV[0] = torch.device('cuda:0')
    x, y = gridded_case(1, 512, 512, 5)
    assert _min_gap(x, y) > 0.5 / (512 * 512)
    _check_f64(x, y, dict(reduction='none'), dev='cuda:0')


# --------------------------------------------------------------------------- #
# 4. ties: only what does not depend on the order inside a run of equal errors
# --------------------------------------------------------------------------- #
def _sorted_state(work, P, C):
    """the last class's sorted (error, foreground flag, pixel) and per-pixel g out of `work` (include/ledn.h: hdr[4],
    the gradient [P][C], key0, key1, idx0, idx1, g -- each padded to a multiple of four words)"""
    al = lambda v: (v + 3) & ~3          # noqa: E731
    w = work.cpu()
    o = 4 + al(P * C)
    sk = w[o:o + P].view(torch.int32).long()
    idx = w[o + 2 * al(P):o + 2 * al(P) + P].view(torch.int32).long()
    g = w[o + 4 * al(P):o + 4 * al(P) + P].double()
    key = 0x7F000002 - sk
    keep = key != 0
    k1 = key[keep] - 1
    e = (k1 >> 1).to(torch.int32).view(torch.float32).double()
    return e, (k1 & 1).double(), idx[keep], g, idx[~keep]


def _tie_inputs(which):
    g = torch.Generator().manual_seed(41)
    N, C, H, Wd = 2, 2, 37, 53
    y = _labels(N, C, H, Wd, g)
    x = torch.zeros(N, C, H, Wd) if which == 'zeros' else (2.0 * torch.randn((N, C, H, Wd), generator=g)).bfloat16().float()
    return x, y


@pytest.mark.parametrize('which', ['zeros', 'bf16'])
def test_lovasz_with_ties(be, which):
    from led_net_amd import ops_train as T
    x, y = _tie_inputs(which)
    N, C, H, Wd = x.shape
    P = N * H * Wd
    kw = dict(reduction='none')
    lg, yd = nhwc(x), D(y)
    with pytest.MonkeyPatch.context() as m:          # (zero-filled allocations: the WHOLE work buffer is compared)
        m.setattr(torch, 'empty', torch.zeros)
        first, second = T.lovasz_loss_fwd(lg, yd, **_fwd_kwargs(kw)), T.lovasz_loss_fwd(lg, yd, **_fwd_kwargs(kw))
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), 'two calls differ'
    out, work = first
    d1 = T.lovasz_loss_bwd(lg, yd, work, out, D(torch.ones(1)))
    d2 = T.lovasz_loss_bwd(lg, yd, second[1], second[0], D(torch.ones(1)))
    assert torch.equal(d1, d2) and bool(torch.isfinite(d1).all())
    # the loss: the f64 restatement on the f32-rounded probabilities
    p32 = torch.softmax(x, dim=1)
    want = ref_lovasz(x.double(), y, probs=p32.double(), **kw)
    print(which, 'loss', float(out[0]), float(want))
    close(out[0], want, 1e-4, 1e-6, 'loss')
    # the sorted order of the last class (1): errors descending, those of |fg - p|, every valid pixel once
    e, fg, pix, gpix, ignored = _sorted_state(work, P, C)
    yv = y.reshape(-1)
    assert bool((e[1:] <= e[:-1]).all()), 'errors not in descending order'
    assert sorted(pix.tolist()) == torch.nonzero(yv != 255).reshape(-1).tolist()
    assert sorted(ignored.tolist()) == torch.nonzero(yv == 255).reshape(-1).tolist()
    assert torch.equal(fg, (yv[pix] == 1).double())
    e_want = ((yv == 1).double() - p32.permute(0, 2, 3, 1).reshape(-1, C)[:, 1].double()).abs()[pix]
    torch.testing.assert_close(e, e_want, rtol=0, atol=2e-7)
    n_runs = int((e[1:] != e[:-1]).sum()) + 1
    assert n_runs < len(e), 'no ties in this input'
    assert bool((gpix[ignored] == 0).all())
    # every run of equal errors: the sum of dL/de over it is the Jaccard index after the run minus the one before it
    G = fg.sum()
    J = 1.0 - (G - fg.cumsum(0)) / (G + (1 - fg).cumsum(0))
    gs = gpix[pix].cumsum(0)
    ends = torch.cat([torch.nonzero(e[1:] != e[:-1]).reshape(-1), torch.tensor([len(e) - 1])])
    run_g = gs[ends] - torch.cat([torch.zeros(1, dtype=torch.float64), gs[ends[:-1]]])
    run_j = J[ends] - torch.cat([torch.zeros(1, dtype=torch.float64), J[ends[:-1]]])
    # (g is f32: 2^-23 relative per element, and the run sums are differences of the running f64 sum of up to P of them)
    torch.testing.assert_close(run_g, run_j, rtol=1e-5, atol=1e-9)


def test_lovasz_all_pixels_ignored(be):
    x, y = _tie_inputs('bf16')
    y[:] = 255
    for kw in (dict(reduction='none'), dict(classes='all', reduction='none'), dict(per_image=True)):
        out, work, dscore = _run_kernels(x, y, kw)
        assert float(out[0]) == 0.0 and float(out[3]) == 0.0 and bool(torch.isfinite(out).all())
        assert bool((dscore == 0).all())
    y[0, 5:, :] = 1          # image 1 stays without a valid pixel: its loss is 0, the mean still divides by 2
    out, work, dscore = _run_kernels(x, y, dict(per_image=True))
    one = ref_lovasz(x[:1].double(), y[:1], per_image=True)
    close(out[0], 0.5 * one, 1e-4, 1e-6, 'one image without a valid pixel')
    assert bool((dscore[1] == 0).all()) and bool(torch.isfinite(dscore).all())


def test_lovasz_label_beyond_the_classes_is_background(be):
    """labels C and C + 7 (not ignore_index) are valid pixels, background for every class, as in the reference"""
    x, y = separated_case(1, 3, 16, 24, 6)
    y[0, 3, :4] = torch.tensor([3, 10, 3, 10])
    x, y = _separate_again(x, y)
    _check_f64(x, y, dict(classes='all', reduction='none'))


# --------------------------------------------------------------------------- #
# 5. LEDHead.loss_by_feat
# --------------------------------------------------------------------------- #
_LV = dict(type='LovaszLoss', reduction='none', loss_weight=0.4)
_LV_PI = dict(type='LovaszLoss', per_image=True, class_weight=[0.7, 1.6], loss_weight=1.0)
_CE = dict(type='CrossEntropyLoss', avg_non_ignore=True, loss_weight=1.0)
_OHEM0 = dict(type='OhemCrossEntropy', thres=0.9, min_kept=300, loss_weight=1.0)
PAIRS = {'ce_lovasz': (_CE, _LV), 'lovasz_ce': (_LV_PI, _CE), 'ohem_lovasz': (_OHEM0, _LV), 'lovasz_lovasz': (_LV, _LV_PI)}


@pytest.mark.parametrize('hw', [(32, 40), (31, 37)], ids=['fold', 'generic_odd'])
@pytest.mark.parametrize('pair', list(PAIRS))
def test_led_head_loss_by_feat_with_lovasz(be, monkeypatch, pair, hw):
    """loss_by_feat against the same losses applied to separately computed fused logits: the Lovasz entry on the
    full-resolution fuse_loss(...) output (never folded), the other entry on its folded (exact 2x) or generic form;
    acc_seg is entry 0's, and a Lovasz entry reports the accuracy a CrossEntropyLoss reports on the same logits"""
    import led_net_amd as L
    from led_net_amd import ops_train as T, train
    H, Wd = hw
    fold = H % 2 == 0 and Wd % 2 == 0
    head, ins, _, label, samples = TS._head_case(PAIRS[pair], hw)
    spy = _Spy(monkeypatch)
    out = head.loss_by_feat(tuple(t.permute(0, 3, 1, 2) for t in ins), samples)
    (out['loss_context'] + 0.5 * out['loss_spatial']).backward()
    got = spy.take()
    up = '_up' if fold else ''
    fam = {'LovaszLoss': 'ledn_lovasz_loss', 'CrossEntropyLoss': f'ledn_ce_loss{up}', 'OhemCrossEntropy': f'ledn_ohem_ce{up}'}
    names = [fam[c['type']] for c in PAIRS[pair]]
    assert got[:2] == [n + '_fwd' for n in names] and sorted(got[2:]) == sorted(n + '_bwd' for n in names), got
    # the same, entry by entry
    ins2 = [t.detach().clone().requires_grad_(True) for t in ins]
    xc, xs, h1, h2 = ins2
    y = D(label.squeeze(1).contiguous())
    want, accs = [], []
    for crit, logit in zip(head.loss_decode, (xc, xs)):
        lovasz = isinstance(crit, L.LovaszLoss)
        full = train.fuse_loss(logit, h1, h2, hw)
        if lovasz:
            want.append(crit(full.permute(0, 3, 1, 2), y, ignore_index=255))
        elif isinstance(crit, L.OhemCrossEntropy):
            fn, src = (train.OhemUpFn, train.fuse_loss_half(logit, h1, h2, hw)) if fold else (train.OhemFn, full)
            want.append(fn.apply(src, y, crit.thresh, crit.min_kept, crit.loss_weight, crit.ignore_label, None)[0])
        else:
            src = train.fuse_loss_half(logit, h1, h2, hw) if fold else full
            want.append(train.seg_loss_apply(crit, src, y, fold, 255)[0])
        accs.append(T.ce_loss_fwd(full.detach(), y, ignore_index=255)[0][1])
    (want[0] + 0.5 * want[1]).backward()
    for key, crit, w in (('loss_context', head.loss_decode[0], want[0]), ('loss_spatial', head.loss_decode[1], want[1])):
        if isinstance(crit, L.LovaszLoss):          # bit for bit: the same kernels on the same logits
            assert torch.equal(out[key].reshape(()), w.detach().reshape(())), key
        else:          # (outside deterministic mode the OHEM kernels end in float atomics: the folded-vs-generic bound)
            close(out[key].reshape(()), w.detach().reshape(()), 2e-6, 1e-8, key)
    if isinstance(head.loss_decode[0], L.LovaszLoss):
        assert torch.equal(out['acc_seg'].reshape(()), accs[0].reshape(())), 'acc_seg is not the CE accuracy of the context logits'
    else:          # (a folded entry 0 interpolates inside its kernel: a tie of the two logits may fall the other way)
        close(out['acc_seg'].reshape(()), accs[0].reshape(()), 1e-5, 1e-4, 'acc_seg')
    for name, t, r in zip(('xc', 'xs', 'h1', 'h2'), ins, ins2):
        close(t.grad, r.grad, 1e-5, 1e-9, 'd/d' + name)


def test_entries_without_lovasz_keep_their_launches(be, monkeypatch):
    """a loss_decode without a LovaszLoss issues what it issued before LovaszLoss existed, and nothing of lovasz.hip"""
    want = {('ohem', (32, 40)): ['ledn_ohem2_up_fwd', 'ledn_ohem2_up_bwd'],
            ('ce_dice', (32, 40)): ['ledn_ce_loss_up_fwd', 'ledn_dice_loss_up_fwd', 'ledn_ce_loss_up_bwd', 'ledn_dice_loss_up_bwd'],
            ('ce_dice', (31, 37)): ['ledn_ce_loss_fwd', 'ledn_dice_loss_fwd', 'ledn_ce_loss_bwd', 'ledn_dice_loss_bwd']}
    pairs = {'ohem': (_OHEM0, dict(_OHEM0, loss_weight=0.4)), 'ce_dice': (_CE, dict(type='DiceLoss', loss_weight=0.4))}
    for (pair, hw), names in want.items():
        head, ins, _, _, samples = TS._head_case(pairs[pair], hw)
        spy = _Spy(monkeypatch)
        out = head.loss_by_feat(tuple(t.permute(0, 3, 1, 2) for t in ins), samples)
        (out['loss_context'] + out['loss_spatial']).backward()
        got = spy.take()
        assert got[:len(names) // 2] == names[:len(names) // 2] and sorted(got) == sorted(names), (pair, hw, got)
        assert not any('lovasz' in n for n in got)
        monkeypatch.undo()


# --------------------------------------------------------------------------- #
# 6. the wrappers' and the modules' argument checks
# --------------------------------------------------------------------------- #
def test_wrappers_validate_their_arguments(be):
    import led_net_amd as L
    from led_net_amd import _lib, ops_train as T
    from led_net_amd.ops import LednError
    lg = D(torch.randn(1, 8, 8, 5))
    y5 = D(torch.randint(0, 5, (1, 8, 8)))
    for bad in (lambda: T.lovasz_loss_fwd(lg.double(), y5), lambda: T.lovasz_loss_fwd(lg, y5.int()),
                lambda: T.lovasz_loss_fwd(lg, D(torch.zeros(1, 8, 9, dtype=torch.int64))),
                lambda: T.lovasz_loss_fwd(lg, y5, class_weight=W([1.0, 2.0])),
                lambda: T.lovasz_loss_fwd(lg, y5, class_weight=[1.0] * 5),
                lambda: T.lovasz_loss_fwd(lg, y5, classes=[5]), lambda: T.lovasz_loss_fwd(lg, y5, classes=[1, 1]),
                lambda: T.lovasz_loss_fwd(lg, y5, classes=[]), lambda: T.lovasz_loss_fwd(lg, y5, classes='some'),
                lambda: T.lovasz_loss_fwd(lg, y5, classes=[1.0]), lambda: T.lovasz_loss_fwd(lg, y5, reduction='none'),
                lambda: T.lovasz_loss_fwd(D(torch.randn(1, 8, 8, 1)), y5)):
        with pytest.raises(LednError):
            bad()
    out, work = T.lovasz_loss_fwd(lg, y5)
    assert bool(torch.isfinite(out).all())
    with pytest.raises(LednError, match='work'):
        T.lovasz_loss_bwd(lg, y5, work[:64], out, D(torch.ones(1)))          # a work buffer that is not this call's
    with pytest.raises(LednError, match='work'):
        T.lovasz_loss_bwd(lg, y5, work.double(), out, D(torch.ones(1)))
    sc = lg.permute(0, 3, 1, 2)
    with pytest.raises(ValueError, match='class_weight has 2 entries'):
        L.MODELS.build(dict(type='LovaszLoss', reduction='none', class_weight=[1.0, 2.0])).to(TS._DEV[0])(sc, y5)
    with pytest.raises(ValueError, match='classes'):
        L.MODELS.build(dict(type='LovaszLoss', reduction='none', classes=[1, 7])).to(TS._DEV[0])(sc, y5)
    # the C entry points themselves: sizes outside the limits
    lib = _lib.get_lib()
    assert lib.cdll.ledn_lovasz_work_bytes(2, 64, 1, 0) == 0 and lib.cdll.ledn_lovasz_work_bytes(2, 1 << 30, 2, 0) == 0
    n0, n1 = lib.cdll.ledn_lovasz_work_bytes(2, 5000, 3, 0), lib.cdll.ledn_lovasz_work_bytes(2, 5000, 3, 1)
    assert n0 >= (20 + 4 * 3) * 10000 and n1 >= n0 and n0 % 4 == 0
    rc = lib.cdll.ledn_lovasz_loss_fwd(lg.data_ptr(), y5.data_ptr(), 1, 64, 5, None, None, 0, 2, 0, 0, 255, 1.0,
                                       work.data_ptr(), out.data_ptr(), None)
    assert rc != 0          # mode 2 without a list
