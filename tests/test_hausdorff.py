"""HuasdorffDisstanceLoss (the reference's spelling) through csrc/hausdorff.hip -- an exact squared Euclidean distance
transform on the device and the distance-weighted squared probability error on top of it -- and its way up to
LEDHead(loss_decode=[...]).

Checked against (1) an integer brute force of the transform (and a separable numpy form, itself checked against the
brute force, for the wide case), (2) fixtures from the reference with scipy under it (tests/golden/g25_hausdorff_*;
gen_golden_hausdorff.py), (3) a statement-for-statement restatement of the reference on f64 tensors under torch
autograd with the brute-force transform in place of scipy, (4) construction through the registry and the rejected
arguments, the wrappers' argument checks, (5) LEDHead.loss_by_feat.  The whole training step and the CLI are in
test_hausdorff_step.py.  No test imports scipy or the reference.

Tolerances.  Loss 1e-4 / 1e-6 and accuracy 1e-5 / 1e-4 are the project's (test_seg_losses.py).  Gradient against the
f64 restatement: the project's 1e-3 / 1e-8, the atol relative to the gradient's scale (times its largest entry: D reaches
H^2 + W^2, so the gradient has no fixed size).  Gradient against the REFERENCE's f32 fixtures: rtol 1e-3 and
atol = REF_GRAD_ATOL = 4 x the largest absolute difference between the reference's own f32 gradient (gin/score of the
fixtures) and the f64 restatement's on the same inputs.  Measured over the five fixtures (largest |difference| /
largest |gradient entry|): blobs 9.1e-10 / 5.1e-3, sum_w04 3.8e-10 / 2.2e-3, c5 4.3e-9 / 1.6e-2, 48x40 9.0e-10 /
3.4e-3, full_and_empty 4.71e-8 / 1.1e-2 (the reference's f32 softmax, the f32 cast of its distances and its f32 product
D * delta; D reaches 3 825 there, 81 .. 394 in the others); the largest is 4.714e-8, so REF_GRAD_ATOL = 1.89e-7.
test_hausdorff_golden prints the same figures, and the kernels' own, and asserts that the measurement still holds."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import Fixture, golden_names
import test_seg_losses as TS
from test_seg_losses import CFG, ROOT, D, close, nchw, nhwc, _Spy

HD_CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_hausdorff_config.py')
REF_GRAD_ATOL = 1.89e-7


@pytest.fixture(autouse=True)
def _track_device(request):          # (test_seg_losses.D / nhwc follow the backend of THIS module's tests too)
    TS._DEV[0] = request.getfixturevalue('be').dev if 'be' in request.fixturenames else torch.device('cpu')
    yield


# --------------------------------------------------------------------------- #
# the transform in numpy: brute force, and the separable form for sizes the brute force cannot hold
# --------------------------------------------------------------------------- #
def _ghost(H, Wd):
    """what scipy returns for a mask without a background pixel: the squared distance to row -1, column 0"""
    yy, xx = np.mgrid[0:H, 0:Wd].astype(np.int64)
    return (yy + 1) ** 2 + xx ** 2


def brute_edt_sq(mask):
    """[H,W] bool (True = foreground) -> int64 [H,W]: min over ALL background pixels of dy^2 + dx^2; 0 on background"""
    mask = np.asarray(mask, dtype=bool)
    H, Wd = mask.shape
    ys, xs = np.nonzero(~mask)
    if len(ys) == 0:
        return _ghost(H, Wd)
    yy, xx = np.mgrid[0:H, 0:Wd].astype(np.int32)
    out = np.empty((H, Wd), dtype=np.int64)
    for y0 in range(0, H, 8):          # (row chunks bound the [rows, W, #background] temporary)
        dy = yy[y0:y0 + 8, :, None] - ys.astype(np.int32)
        dx = xx[y0:y0 + 8, :, None] - xs.astype(np.int32)
        out[y0:y0 + 8] = (dy * dy + dx * dx).min(axis=2)
    return out


def sep_edt_sq(mask):
    """the same by columns, then rows: g(x, y) = the vertical distance to the nearest background pixel of column x (none:
    infinite), d2(x, y) = min_x' (x - x')^2 + g(x', y)^2"""
    mask = np.asarray(mask, dtype=bool)
    H, Wd = mask.shape
    if mask.all():
        return _ghost(H, Wd)
    INF = np.int64(1) << 40
    g = np.full((H, Wd), INF, dtype=np.int64)
    run = np.full(Wd, INF, dtype=np.int64)
    for y in range(H):
        run = np.where(mask[y], np.minimum(run + 1, INF), 0)
        g[y] = run
    run = np.full(Wd, INF, dtype=np.int64)
    for y in range(H - 1, -1, -1):
        run = np.where(mask[y], np.minimum(run + 1, INF), 0)
        g[y] = np.minimum(g[y], run)
    g2 = np.where(g >= INF, INF, g * g)
    x = np.arange(Wd, dtype=np.int64)
    dx2 = (x[:, None] - x[None, :]) ** 2          # [x, x']
    out = np.empty((H, Wd), dtype=np.int64)
    for y in range(H):
        out[y] = (dx2 + g2[y][None, :]).min(axis=1)
    return out


def _masks(H, Wd, seed):
    """the masks of the issue for one shape, [K,H,W] bool"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = np.mgrid[0:H, 0:Wd]
    ms = [np.zeros((H, Wd), bool), np.ones((H, Wd), bool)]
    for cy, cx in ((0, 0), (0, Wd - 1), (H - 1, 0), (H - 1, Wd - 1)):          # one background pixel, in each corner
        m = np.ones((H, Wd), bool)
        m[cy, cx] = False
        ms.append(m)
    ms.append((yy + xx) % 2 == 0)
    ms.append((torch.rand((H, Wd), generator=g) < 0.05).numpy())
    ms.append((torch.rand((H, Wd), generator=g) < 0.95).numpy())
    m = np.zeros((H, Wd), bool)          # a filled rectangle wider than a wave (where the shape allows: 70 of 83 columns)
    m[H // 8:H - H // 8 if H > 8 else H, 6:max(7, Wd - 7)] = True
    ms.append(m)
    ms.append(np.broadcast_to((xx[0] % 7) < 4, (H, Wd)).copy())          # full columns next to empty ones
    m = np.ones((H, Wd), bool)          # ... and every column full but the last one, which has ONE background pixel
    m[H // 2, Wd - 1] = False
    ms.append(m)
    return np.stack(ms)


def _edt(masks):
    from led_net_amd import ops_train as T
    return T.edt_sq(D(torch.from_numpy(np.ascontiguousarray(masks)).to(torch.uint8))).cpu().numpy()


# --------------------------------------------------------------------------- #
# 1. the transform
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('hw', [(1, 1), (1, 70), (70, 1), (37, 83)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_edt_sq_equals_the_brute_force(be, hw):
    ms = _masks(*hw, seed=7)
    got = _edt(ms)
    assert got.dtype == np.int32 and got.shape == ms.shape
    for k, m in enumerate(ms):
        want = brute_edt_sq(m)
        assert np.array_equal(sep_edt_sq(m), want), f'mask {k}: the separable numpy form disagrees with the brute force'
        assert np.array_equal(got[k], want), f'mask {k} of {hw}: {np.abs(got[k] - want).max()} off'
    assert np.array_equal(got[1], _ghost(*hw)) and not got[0].any()


def test_edt_sq_three_images_three_masks(be):
    ms = _masks(37, 83, seed=8)[[8, 1, 9]]          # 95 % foreground, all foreground (the ghost form), the rectangle
    got = _edt(ms)
    for k in range(3):
        assert np.array_equal(got[k], brute_edt_sq(ms[k])), k
    one = _edt(ms[2:3])
    assert np.array_equal(one[0], got[2])
    from led_net_amd import ops_train as T
    assert np.array_equal(T.edt_sq(D(torch.from_numpy(ms.copy()))).cpu().numpy(), got)          # a bool mask


def test_edt_sq_wide_rows(be):
    """2 x 24 x 1100: W beyond one workgroup's 256 lanes and no multiple of 64; image 1 is the search's worst case (one
    background pixel in a corner: every pixel walks to the far end)"""
    g = torch.Generator().manual_seed(9)
    ms = np.stack([(torch.rand((24, 1100), generator=g) < 0.97).numpy(), np.ones((24, 1100), bool)])
    ms[0, 4:20, 300:900] = True
    ms[1, 23, 0] = False
    got = _edt(ms)
    for k in range(2):
        assert np.array_equal(got[k], sep_edt_sq(ms[k])), k
    assert got[1, 0, 1099] == 23 * 23 + 1099 * 1099


# --------------------------------------------------------------------------- #
# the reference's forward, statement for statement, in the dtype of `pred` (huasdorff_distance_loss.py:14-74,109-156);
# the squared maps are the exact integers (the reference squares the f32 cast of an f64 square root)
# --------------------------------------------------------------------------- #
def ref_dtm_sq(img_gt, pred, edt):
    fg = torch.zeros_like(pred)
    for b in range(pred.shape[0]):
        posmask = (img_gt[b].cpu() % 256) != 0          # (.byte())
        if bool(posmask.any()):
            d2 = torch.from_numpy(edt(posmask.numpy())).to(pred)
            for c in range(1, pred.shape[1]):
                fg[b][c] = d2
    return fg


def ref_hausdorff(pred, target, reduction='mean', loss_weight=1.0, ignore_index=255, edt=brute_edt_sq, seg_mask=None):
    """HuasdorffDisstanceLoss.forward; seg_mask: a label map to use instead of argmax(softmax(pred)) (the step test's
    bounds)"""
    pred_soft = F.softmax(pred, dim=1)
    valid_mask = (target != ignore_index).long()
    target = target * valid_mask
    with torch.no_grad():
        gt_dtm2 = ref_dtm_sq(target, pred_soft, edt)
        seg_dtm2 = ref_dtm_sq(pred_soft.argmax(dim=1) if seg_mask is None else seg_mask, pred_soft, edt)
    total_loss = 0
    num_class = pred_soft.shape[1]
    for i in range(1, num_class):
        if i != ignore_index:
            delta_s = (pred_soft[:, i, ...] - target.to(pred.dtype)) ** 2
            dtm = seg_dtm2[:, i, ...] + gt_dtm2[:, i, ...]
            hd_loss = (delta_s * dtm).mean()
        total_loss = total_loss + hd_loss
    return loss_weight * (total_loss / num_class)          # (mean, sum and none of a scalar: the scalar)


def _run_kernels(score, tgt, loss_weight=1.0, ignore_index=255, dloss=1.0):
    """ops_train forward + backward on NCHW `score` -> (out, work, d score NCHW on the CPU)"""
    from led_net_amd import ops_train as T
    lg, y = nhwc(score), D(tgt.contiguous())
    out, work = T.hausdorff_loss_fwd(lg, y, loss_weight=loss_weight, ignore_index=ignore_index)
    dl = T.hausdorff_loss_bwd(lg, y, work, out, D(torch.tensor([dloss])))
    return out, work, nchw(dl)


def blob_labels(N, C, H, Wd, g, ignore=True):
    """a few filled rectangles and discs of the classes 1 .. C-1 on background 0, one filled rectangle of 255"""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(Wd), indexing='ij')
    y = torch.zeros((N, H, Wd), dtype=torch.int64)
    for b in range(N):
        for k in range(3):
            cy, cx = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, Wd, (1,), generator=g))
            r = int(torch.randint(max(2, min(H, Wd) // 6), max(3, min(H, Wd) // 3), (1,), generator=g))
            m = ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r) if k % 2 else (((yy - cy).abs() <= r) & ((xx - cx).abs() <= r))
            y[b][m] = 1 + (b + k) % (C - 1)
        if ignore:
            y[b, H // 3:H // 3 + max(1, H // 4), Wd // 5:Wd // 5 + max(1, Wd // 3)] = 255
    return y


def blob_case(N, C, H, Wd, seed, ignore=True):
    """labels as above; logits that follow the labels moved by (2, -3) pixels, margin 2, noise 0.6"""
    g = torch.Generator().manual_seed(seed)
    y = blob_labels(N, C, H, Wd, g, ignore)
    pred = torch.roll(torch.where(y == 255, torch.zeros_like(y), y), shifts=(2, -3), dims=(1, 2))
    x = 0.6 * torch.randn((N, C, H, Wd), generator=g)
    x.scatter_add_(1, pred.unsqueeze(1), torch.full((N, 1, H, Wd), 2.0))
    return x, y


# --------------------------------------------------------------------------- #
# 2. the reference's numbers
# --------------------------------------------------------------------------- #
GOLDEN = golden_names('g25_hausdorff_')


def test_golden_set_is_complete():
    assert {n[len('g25_hausdorff_'):] for n in GOLDEN} >= {'blobs', 'sum_w04', 'c5', '48x40', 'full_and_empty'}
    for n in GOLDEN:
        assert Fixture(n).ins['target'].numel() <= 8192
    fx = Fixture('g25_hausdorff_full_and_empty')
    y, am = fx.ins['target'], fx.ins['score'].argmax(1)
    assert bool((y[0] != 0).all()) and bool((am[1] != 0).all()) and not bool(y[2].any()) and not bool(am[2].any())
    assert sorted(set(Fixture('g25_hausdorff_c5').ins['target'].reshape(-1).tolist()) - {255}) == [0, 1, 2, 3, 4]
    kw = Fixture('g25_hausdorff_sum_w04').meta['kwargs']
    assert kw == dict(loss_weight=0.4, reduction='sum') and tuple(Fixture('g25_hausdorff_48x40').ins['target'].shape[1:]) == (48, 40)


@pytest.mark.parametrize('name', GOLDEN)
def test_hausdorff_golden(be, name):
    """the kernels give the fixture's loss, accuracy and gradient; so does the module through autograd; the f64
    restatement gives the fixture's numbers too (this is where REF_GRAD_ATOL was measured)"""
    import led_net_amd as L
    fx = Fixture(name)
    kw, ign = fx.meta['kwargs'], fx.meta['ignore_index']
    score, tgt = fx.ins['score'], fx.ins['target']
    assert ign == 255
    if 'full_and_empty' not in name:
        assert 0.05 <= float((tgt == 255).float().mean()) <= 0.2
    assert torch.equal(score.argmax(1), torch.softmax(score, 1).argmax(1))          # no argmax ties in the fixtures
    xd = score.double().requires_grad_(True)
    want64 = ref_hausdorff(xd, tgt, **kw)
    want64.backward()
    ref_err = float((fx.gin['score'].double() - xd.grad).abs().max())
    close(want64, fx.outs['loss'].reshape(()), 1e-5, 1e-7, name + ': restatement vs fixture')
    lw = kw.get('loss_weight', 1.0)
    out, work, dscore = _run_kernels(score, tgt, loss_weight=lw)
    print(name, 'loss', float(out[0]), 'want', float(fx.outs['loss']), 'acc', float(out[1]), float(fx.outs['acc']),
          'reference f32 vs f64 gradient', ref_err, 'kernels vs fixture', float((dscore - fx.gin['score']).abs().max()),
          'max |d|', float(fx.gin['score'].abs().max()))
    assert 4 * ref_err <= REF_GRAD_ATOL * 1.0001
    close(out[0], fx.outs['loss'].reshape(()), 1e-4, 1e-6, name + ' loss')
    close(out[1], fx.outs['acc'].reshape(()), 1e-5, 1e-4, name + ' acc')
    assert float(out[2]) == float(score.shape[1] * tgt.numel()) and float(out[3]) == float((tgt != 255).sum())
    close(dscore, fx.gin['score'], 1e-3, REF_GRAD_ATOL, name + ' dscore')
    crit = L.MODELS.build(dict(type='HuasdorffDisstanceLoss', **kw)).to(TS._DEV[0])
    sc = nhwc(score).requires_grad_(True)
    loss = crit(sc.permute(0, 3, 1, 2), D(tgt), ignore_index=ign)
    close(loss, fx.outs['loss'].reshape(()), 1e-4, 1e-6, name + ' module loss')
    (2.0 * loss).backward()
    close(nchw(sc.grad), 2.0 * fx.gin['score'], 1e-3, 2 * REF_GRAD_ATOL, name + ' module dscore')


# --------------------------------------------------------------------------- #
# 3. against the f64 restatement under autograd
# --------------------------------------------------------------------------- #
def _check_f64(x, y, loss_weight=1.0, dloss=1.0, ignore_index=255):
    xd = x.double().requires_grad_(True)
    want = ref_hausdorff(xd, y, loss_weight=loss_weight, ignore_index=ignore_index)
    (dloss * want).backward()
    out, work, dscore = _run_kernels(x, y, loss_weight=loss_weight, ignore_index=ignore_index, dloss=dloss)
    gw = xd.grad
    scale = float(gw.abs().max())
    print(tuple(x.shape), 'loss', float(out[0]), float(want.detach()), 'max |d| err', float((dscore - gw).abs().max()),
          'max |d|', scale)
    close(out[0], want.detach(), 1e-4, 1e-6, 'loss')
    assert scale > 0
    torch.testing.assert_close(dscore.double(), gw, rtol=1e-3, atol=1e-8 * scale, msg=lambda m: f'dscore: {m}')
    # D in the work buffer: the two transforms of the masks, bit for bit
    N, C, H, Wd = x.shape
    Dm = work[4:4 + N * H * Wd].view(torch.int32).reshape(N, H, Wd).cpu().numpy()
    ys = torch.where(y == ignore_index, torch.zeros_like(y), y)
    for b in range(N):
        want_d = brute_edt_sq((x[b].argmax(0) != 0).numpy()) + brute_edt_sq((ys[b] != 0).numpy())
        assert np.array_equal(Dm[b], want_d), f'D of image {b}'
    return out


@pytest.mark.parametrize('shape,seed', [((1, 2, 24, 37), 1), ((2, 2, 31, 45), 2), ((2, 3, 33, 29), 3), ((1, 19, 16, 21), 4)],
                         ids=['n1_c2', 'n2_c2', 'n2_c3', 'n1_c19'])
def test_hausdorff_vs_f64(be, shape, seed):
    x, y = blob_case(*shape, seed)
    assert bool((y == 255).any()) and len(set(y.reshape(-1).tolist()) - {0, 255}) >= 1
    out = _check_f64(x, y)
    assert float(out[2]) == float(shape[1] * y.numel())


def test_hausdorff_vs_f64_more_than_one_tile_dloss_and_weight(be):
    """2 x 2 x 40 x 53 = 4 240 pixels (three workgroups of the streaming passes, a partial last one), dloss = -0.7,
    loss_weight = 0.4, the loss's ignore_index 7 (255 labels are then raw targets of 255, as in the reference)"""
    x, y = blob_case(2, 2, 40, 53, 5)
    _check_f64(x, y, loss_weight=0.4, dloss=-0.7)
    y2 = torch.where(y == 255, torch.full_like(y, 7), y)
    _check_f64(x, y2, ignore_index=7)
    y3 = y.clone()
    y3[y3 == 255] = 1
    a = _run_kernels(x, y, ignore_index=9)          # 255 is now a raw target value: foreground, huge errors
    b = _check_f64(x, y, ignore_index=9)
    assert torch.equal(a[0], b) and float(a[0][0]) > 100 * float(_run_kernels(x, y3)[0][0])


def test_all_three_reductions_give_the_same_number(be):
    import led_net_amd as L
    x, y = blob_case(2, 2, 24, 37, 6)
    sc = nhwc(x)
    got = [L.MODELS.build(dict(type='HuasdorffDisstanceLoss', reduction=r, loss_weight=0.4)).to(TS._DEV[0])(
        sc.permute(0, 3, 1, 2), D(y)) for r in ('mean', 'sum', 'none')]
    assert got[0].dim() == 0 and torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    close(got[0], ref_hausdorff(x.double(), y, loss_weight=0.4), 1e-4, 1e-6, 'loss')
    # a call-time ignore_index is the accuracy's, never the loss's (the reference swallows it in **kwargs)
    crit = L.MODELS.build(dict(type='HuasdorffDisstanceLoss', loss_weight=0.4)).to(TS._DEV[0])
    assert torch.equal(crit(sc.permute(0, 3, 1, 2), D(y), ignore_index=0), got[0])


# --------------------------------------------------------------------------- #
# 4. construction and checks
# --------------------------------------------------------------------------- #
def test_hausdorff_builds_with_the_reference_defaults_and_rejects_what_is_not_built():
    import led_net_amd as L
    m = L.MODELS.build(dict(type='HuasdorffDisstanceLoss'))
    assert isinstance(m, L.HuasdorffDisstanceLoss) and m.loss_name == 'loss_huasdorff_disstance'
    assert list(m.state_dict()) == [] and list(m.parameters()) == [] and list(m.buffers()) == []
    assert (m.reduction, m.class_weight, m.loss_weight, m.ignore_index) == ('mean', None, 1.0, 255)
    m = L.MODELS.build(dict(type='HuasdorffDisstanceLoss', reduction='sum', loss_weight=0.4, ignore_index=7, loss_name='loss_x',
                            some_other_key=1))          # (**kwargs, as the reference)
    assert (m.reduction, m.loss_weight, m.ignore_index, m.loss_name) == ('sum', 0.4, 7, 'loss_x')
    for cfg, exc, word in ((dict(class_weight=[0.7, 1.6]), NotImplementedError, 'class_weight'),
                           (dict(class_weight='weights.npy'), TypeError, 'class_weight'),
                           (dict(reduction='max'), ValueError, 'reduction')):
        with pytest.raises(exc, match=word):
            L.MODELS.build(dict(type='HuasdorffDisstanceLoss', **cfg))
    cfg = L.load_config(HD_CFG)['model']['decode_head']
    head = L.MODELS.build(cfg)
    assert [type(m).__name__ for m in head.loss_decode] == ['CrossEntropyLoss', 'HuasdorffDisstanceLoss']
    assert set(head.state_dict()) == set(L.MODELS.build(L.load_config(CFG)['model']['decode_head']).state_dict())
    hd = dict(type='HuasdorffDisstanceLoss')
    for pair in ((hd, dict(type='DiceLoss')), (dict(type='OhemCrossEntropy'), hd), (hd, hd),
                 (dict(type='LovaszLoss', reduction='none'), hd)):
        cfg['loss_decode'] = [dict(p) for p in pair]
        assert [type(m).__name__ for m in L.MODELS.build(cfg).loss_decode] == [p['type'] for p in pair]

    class ForeignLoss(nn.Module):
        def __init__(self, loss_weight=1.0):
            super().__init__()
    L.MODELS.register_module(name='ForeignLossForHausdorffTest', force=True, module=ForeignLoss)
    cfg['loss_decode'][1] = dict(type='ForeignLossForHausdorffTest')
    with pytest.raises(TypeError, match='HuasdorffDisstanceLoss'):
        L.MODELS.build(cfg)


def test_wrappers_validate_their_arguments(be):
    import led_net_amd as L
    from led_net_amd import _lib, ops_train as T
    from led_net_amd.ops import LednError
    lg = D(torch.randn(1, 8, 8, 5))
    y5 = D(torch.randint(0, 5, (1, 8, 8)))
    one = D(torch.ones(1))
    for bad in (lambda: T.hausdorff_loss_fwd(lg.double(), y5), lambda: T.hausdorff_loss_fwd(lg, y5.int()),
                lambda: T.hausdorff_loss_fwd(lg, D(torch.zeros(1, 8, 9, dtype=torch.int64))),
                lambda: T.hausdorff_loss_fwd(lg[0], y5), lambda: T.hausdorff_loss_fwd(lg.permute(0, 2, 1, 3), y5),
                lambda: T.hausdorff_loss_fwd(D(torch.randn(1, 8, 8, 1)), y5),
                lambda: T.hausdorff_loss_fwd(D(torch.randn(1, 8, 8, 33)), y5),
                lambda: T.hausdorff_loss_fwd(D(torch.zeros(1, 1, 8193, 2)), D(torch.zeros(1, 1, 8193, dtype=torch.int64))),
                lambda: T.edt_sq(D(torch.zeros(1, 1, 8193, dtype=torch.uint8))),
                lambda: T.edt_sq(D(torch.zeros(1, 8, 8, dtype=torch.int32))), lambda: T.edt_sq(D(torch.zeros(8, 8, dtype=torch.uint8))),
                lambda: T.edt_sq(D(torch.zeros(2, 8, 8, dtype=torch.uint8))[:, :, ::2])):
        with pytest.raises(LednError):
            bad()
    with pytest.raises(LednError, match='8192'):
        T.hausdorff_loss_fwd(D(torch.zeros(1, 1, 8193, 2)), D(torch.zeros(1, 1, 8193, dtype=torch.int64)))
    if TS._DEV[0].type == 'cuda':          # the other device
        with pytest.raises(LednError):
            T.hausdorff_loss_fwd(lg.cpu(), y5.cpu())
        with pytest.raises(LednError):
            T.edt_sq(torch.zeros(1, 8, 8, dtype=torch.uint8))
    out, work = T.hausdorff_loss_fwd(lg, y5)
    assert bool(torch.isfinite(out).all())
    with pytest.raises(LednError, match='work'):
        T.hausdorff_loss_bwd(lg, y5, work[:64], out, one)          # a work buffer that is not this call's
    with pytest.raises(LednError, match='work'):
        T.hausdorff_loss_bwd(lg, y5, work.double(), out, one)
    with pytest.raises(LednError):
        T.hausdorff_loss_bwd(lg.double(), y5, work, out, one)
    with pytest.raises(LednError):
        T.hausdorff_loss_bwd(lg, y5[:, :4], work, out, one)
    sc = lg.permute(0, 3, 1, 2)
    for ign in (1, 4):          # ignore_index inside [1, C): at call time
        crit = L.MODELS.build(dict(type='HuasdorffDisstanceLoss', ignore_index=ign))
        with pytest.raises(ValueError, match='ignore_index'):
            crit(sc, y5)
    assert bool(torch.isfinite(L.MODELS.build(dict(type='HuasdorffDisstanceLoss', ignore_index=5))(sc, y5)))
    assert bool(torch.isfinite(L.MODELS.build(dict(type='HuasdorffDisstanceLoss', ignore_index=0))(sc, y5)))
    with pytest.raises(NotImplementedError, match='avg_factor'):
        L.MODELS.build(dict(type='HuasdorffDisstanceLoss'))(sc, y5, avg_factor=3.0)
    # the C entry points themselves: sizes outside the limits
    lib = _lib.get_lib()
    wb = lib.cdll.ledn_hausdorff_work_bytes
    assert wb(2, 64, 64, 1) == 0 and wb(2, 64, 64, 33) == 0 and wb(1, 8, 8193, 2) == 0 and wb(1, 32768, 8, 2) == 0
    n0 = wb(2, 50, 100, 3)
    assert n0 >= 16 + 8 * 10000 and n0 % 4 == 0 and n0 == wb(2, 50, 100, 19)
    rc = lib.cdll.ledn_hausdorff_loss_fwd(lg.data_ptr(), y5.data_ptr(), 1, 8, 8, 40, 255, 255, 1.0, work.data_ptr(),
                                          out.data_ptr(), None)
    assert rc != 0
    m8 = D(torch.zeros(1, 8, 8, dtype=torch.uint8))
    assert lib.cdll.ledn_edt_sq(m8.data_ptr(), 1, 8, 8193, m8.data_ptr(), None) != 0


# --------------------------------------------------------------------------- #
# 5. LEDHead.loss_by_feat
# --------------------------------------------------------------------------- #
_HD = dict(type='HuasdorffDisstanceLoss', loss_weight=0.02)
_CE = dict(type='CrossEntropyLoss', avg_non_ignore=True, loss_weight=1.0)
_OHEM0 = dict(type='OhemCrossEntropy', thres=0.9, min_kept=300, loss_weight=1.0)
PAIRS = {'ce_hd': (_CE, _HD), 'hd_ce': (_HD, _CE), 'ohem_hd': (_OHEM0, _HD), 'hd_ohem': (_HD, _OHEM0)}


@pytest.mark.parametrize('hw', [(32, 40), (31, 37)], ids=['fold', 'generic_odd'])
@pytest.mark.parametrize('pair', list(PAIRS))
def test_led_head_loss_by_feat_with_hausdorff(be, monkeypatch, pair, hw):
    """loss_by_feat against the same losses applied to separately computed fused logits: the Hausdorff entry on the
    full-resolution fuse_loss(...) output (never folded), the other entry on its folded (exact 2x) or generic form;
    acc_seg is entry 0's, and a Hausdorff entry reports the accuracy a CrossEntropyLoss reports on the same logits"""
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
    fam = {'HuasdorffDisstanceLoss': 'ledn_hausdorff_loss', 'CrossEntropyLoss': f'ledn_ce_loss{up}',
           'OhemCrossEntropy': f'ledn_ohem_ce{up}'}
    names = [fam[c['type']] for c in PAIRS[pair]]
    assert got[:2] == [n + '_fwd' for n in names] and sorted(got[2:]) == sorted(n + '_bwd' for n in names), got
    ins2 = [t.detach().clone().requires_grad_(True) for t in ins]
    xc, xs, h1, h2 = ins2
    y = D(label.squeeze(1).contiguous())
    want, accs = [], []
    for crit, logit in zip(head.loss_decode, (xc, xs)):
        full = train.fuse_loss(logit, h1, h2, hw)
        if isinstance(crit, L.HuasdorffDisstanceLoss):
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
        if isinstance(crit, L.HuasdorffDisstanceLoss):          # bit for bit: the same kernels on the same logits
            assert torch.equal(out[key].reshape(()), w.detach().reshape(())), key
        else:          # (outside deterministic mode the OHEM kernels end in float atomics: the folded-vs-generic bound)
            close(out[key].reshape(()), w.detach().reshape(()), 2e-6, 1e-8, key)
    if isinstance(head.loss_decode[0], L.HuasdorffDisstanceLoss):
        assert torch.equal(out['acc_seg'].reshape(()), accs[0].reshape(())), 'acc_seg is not the CE accuracy of the context logits'
    else:          # (a folded entry 0 interpolates inside its kernel: a tie of the two logits may fall the other way)
        close(out['acc_seg'].reshape(()), accs[0].reshape(()), 1e-5, 1e-4, 'acc_seg')
    for name, t, r in zip(('xc', 'xs', 'h1', 'h2'), ins, ins2):
        close(t.grad, r.grad, 1e-5, 1e-9, 'd/d' + name)


def test_a_folded_call_of_the_family_is_refused():
    from led_net_amd import train
    x, y = torch.zeros(1, 4, 4, 2), torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match='no resize-folded form'):
        train.SegLossFn.apply(x, y, 'hausdorff', True, {}, {})
