"""OhemCrossEntropy(class_weight=[...]) through the fused loss kernels (ledn_ohem_ce_w_*, ledn_ohem_ce_up_w_*,
ledn_ohem2_up_w_*): the per-pixel loss is w[y] * CE, the selection (target-class probability, k-th order statistic,
threshold = max(k-th, thres), strict <) does not see the weights, and the mean divides by the NUMBER of selected
pixels (mmseg/models/losses/ohem_cross_entropy_loss.py:62-90).

Checked against (1) fixtures written by the reference's own class (tests/golden/g21_ohemcw_*), (2) the same inputs
without weights (selection bit-identical), (3) the three kernel families against each other, (4) plain torch autograd
through a restatement of the reference's forward, (5) neutral weights and the entry points taken, (6) the module and
LEDHead.loss_by_feat on every dispatch branch, (7) a whole Trainer step (eager = graph replay, run = run, bit for
bit) and (8) the training CLI."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import Fixture, golden_names, slow_on_emu
from oracle import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_test_config.py')
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


def ref_ohem_ce(score, target, thres, min_kept, loss_weight, class_weight=None, ignore_label=255):
    """OhemCrossEntropy.forward with class_weight, statement for statement from
    mmseg/models/losses/ohem_cross_entropy_loss.py:62-90 (score N x C x H x W)."""
    min_kept = max(1, min_kept)
    pred = F.softmax(score, dim=1)
    if class_weight is not None:
        class_weight = score.new_tensor(class_weight)
    else:
        class_weight = None
    pixel_losses = F.cross_entropy(score, target, weight=class_weight, ignore_index=ignore_label,
                                   reduction='none').contiguous().view(-1)
    mask = target.contiguous().view(-1) != ignore_label
    tmp_target = target.clone()
    tmp_target[tmp_target == ignore_label] = 0
    pred = pred.gather(1, tmp_target.unsqueeze(1))
    pred, ind = pred.contiguous().view(-1, )[mask].contiguous().sort()
    if pred.numel() > 0:
        min_value = pred[min(min_kept, pred.numel() - 1)]
    else:
        return score.new_tensor(0.0)
    threshold = max(min_value, thres)
    pixel_losses = pixel_losses[mask][ind]
    pixel_losses = pixel_losses[pred < threshold]
    return loss_weight * pixel_losses.mean()


def close(a, b, rt, at, what=''):
    torch.testing.assert_close(a.detach().cpu().float(), b.cpu().float(), rtol=rt, atol=at, msg=lambda m: f'{what}: {m}')


# --------------------------------------------------------------------------- #
# 1. the reference's own numbers
# --------------------------------------------------------------------------- #
GOLDEN = golden_names('g21_ohemcw_')


def test_golden_set_is_complete():
    assert {n[len('g21_ohemcw_'):] for n in GOLDEN} >= {'k1000', 'k131072', 'k100_confident', 'c5', 'c19', 'zero_one',
                                                        'all_ignored'}


@pytest.mark.parametrize('name', GOLDEN)
def test_ohem_class_weight_golden(be, name):
    """tolerances of test_ops_bwd.test_ohem_golden: loss 1e-4 / 1e-6, gradient 1e-3 / 1e-8"""
    from led_net_amd import ops_train as T
    fx = Fixture(name)
    kw = fx.meta['kwargs']
    score, tgt = fx.ins['score'], fx.ins['target']
    assert len(kw['class_weight']) == score.shape[1]
    lg, cw = nhwc(score), W(kw['class_weight'])
    out, work = T.ohem_ce_fwd(lg, D(tgt.contiguous()), kw['thres'], max(1, kw['min_kept']), kw['loss_weight'],
                              class_weight=cw)
    print(name, 'loss', float(out[0]), 'want', float(fx.outs['loss']))
    close(out[0], fx.outs['loss'].reshape(()), 1e-4, 1e-6, name + ' loss')
    close(out[1], fx.outs['acc'].reshape(()), 1e-5, 1e-4, name + ' acc')
    if 'score' in fx.gin:
        dl = T.ohem_ce_bwd(lg, D(tgt.contiguous()), work, out, D(torch.ones(1)), kw['loss_weight'], class_weight=cw)
        close(nchw(dl), fx.gin['score'], 1e-3, 1e-8, name + ' dscore')
    else:
        assert float(out[0]) == 0.0 and float(out[3]) == 0.0           # every pixel ignored


def test_zero_weight_divides_by_the_count():
    """the fixture with weights [0, 1] tells the two possible divisors apart: the reference's loss is far from the
    weight-normalised mean of the same selected pixels"""
    fx = Fixture('g21_ohemcw_zero_one')
    kw = fx.meta['kwargs']
    got = ref_ohem_ce(fx.ins['score'], fx.ins['target'], kw['thres'], kw['min_kept'], kw['loss_weight'], kw['class_weight'])
    torch.testing.assert_close(got, fx.outs['loss'].reshape(()), rtol=1e-6, atol=0)
    by_count = float(fx.outs['loss'])
    one = ref_ohem_ce(fx.ins['score'], fx.ins['target'], kw['thres'], kw['min_kept'], kw['loss_weight'], None)
    assert by_count < 0.75 * float(one)        # about half of the selected pixels carry weight 0 and still count


# --------------------------------------------------------------------------- #
# 2. + 3. + 4.  selection invariance, the three paths against each other and against torch autograd
# --------------------------------------------------------------------------- #
import test_ohem_fused as TF  # noqa: E402  (CASES and the seeded inputs of the unweighted pair test)

WEIGHTS = [([0.7, 1.6], [1.3, 0.5]), ([0.8, 1.2], None), (None, [0.25, 2.0])]


@pytest.mark.parametrize('cws', WEIGHTS, ids=['both', 'first', 'second'])
@pytest.mark.parametrize('N,Hs,Ws,kept,thr,ignore', TF.CASES)
def test_three_paths_agree_and_selection_is_untouched(be, N, Hs, Ws, kept, thr, ignore, cws):
    from led_net_amd import ops, ops_train as T
    s0, s1, y = TF._inputs(N, Hs, Ws, ignore, 7 + N)
    cfg = [(thr[0], kept[0], 1.0), (thr[1], kept[1], 0.4)]
    H, Wd = 2 * Hs, 2 * Ws
    cwd = (W(cws[0]), W(cws[1]))
    out, work = T.ohem2_up_fwd(D(s0), D(s1), D(y), cfg[0], cfg[1], 255, class_weights=cwd)
    out0, _ = T.ohem2_up_fwd(D(s0), D(s1), D(y), cfg[0], cfg[1], 255)                  # the same pair, unweighted
    out, out0 = out.cpu(), out0.cpu()
    assert torch.equal(out[:, 1:], out0[:, 1:]), (out, out0)          # accuracy, threshold, n_selected: bit-identical
    g = (torch.tensor([0.7]), torch.tensor([1.3]))
    if ignore != 'all':
        d = T.ohem2_up_bwd(D(s0), D(s1), (H, Wd), work, D(out), D(g[0]), D(g[1]), cfg[0][2], cfg[1][2], 255,
                           class_weights=cwd)
    for k, s in enumerate((s0, s1)):
        c = cfg[k]
        # the single resize-folded loss
        o1, w1 = T.ohem_ce_up_fwd(D(s), D(y), c[0], c[1], c[2], 255, class_weight=cwd[k])
        o1u, _ = T.ohem_ce_up_fwd(D(s), D(y), c[0], c[1], c[2], 255)
        assert torch.equal(o1.cpu()[1:], o1u.cpu()[1:]), (o1, o1u)
        assert float(o1[2]) == float(out[k, 2]) and float(o1[3]) == float(out[k, 3]), (o1, out[k])
        if k == 0:
            assert float(o1[1]) == float(out[0, 1])
        # the generic kernel on explicitly resized logits (the product's resize kernel: the taps and the expression of
        # the fold, so that the probabilities, and with them thresholds and counts, are the same numbers)
        lg = ops.bilinear(D(s), (H, Wd))
        o2, w2 = T.ohem_ce_fwd(lg, D(y), c[0], c[1], c[2], 255, class_weight=cwd[k])
        o2u, _ = T.ohem_ce_fwd(lg, D(y), c[0], c[1], c[2], 255)
        assert torch.equal(o2.cpu()[1:], o2u.cpu()[1:]), (o2, o2u)
        assert float(o2[2]) == float(out[k, 2]) and float(o2[3]) == float(out[k, 3]), (o2, out[k])
        if ignore == 'all':
            assert float(out[k, 0]) == 0.0 and float(o1[0]) == 0.0 and float(o2[0]) == 0.0 and float(out[k, 3]) == 0.0
            continue
        want = float(o1[0])
        print(f'loss {k}: pair {float(out[k, 0])!r} single {want!r} generic {float(o2[0])!r}')
        assert abs(float(out[k, 0]) - want) <= 2e-6 * abs(want) + 1e-8
        assert abs(float(o2[0]) - want) <= 2e-6 * abs(want) + 1e-8
        # gradients: pair vs single
        d1 = T.ohem_ce_up_bwd(D(s), D(y), w1, o1, D(g[k]), c[2], 255, class_weight=cwd[k])
        torch.testing.assert_close(d[k].cpu(), d1.cpu(), rtol=1e-5, atol=1e-8)
        # generic backward, pulled through the resize by autograd, vs single
        dl = T.ohem_ce_bwd(lg, D(y), w2, o2, D(g[k]), c[2], 255, class_weight=cwd[k]).cpu()
        sr = s.clone().requires_grad_(True)
        upr = F.interpolate(sr.permute(0, 3, 1, 2), size=(H, Wd), mode='bilinear', align_corners=False)
        upr.backward(dl.permute(0, 3, 1, 2))
        torch.testing.assert_close(sr.grad, d1.cpu(), rtol=1e-5, atol=1e-8)
        # (4) plain torch autograd through the reference's statements
        sr = s.clone().requires_grad_(True)
        upr = F.interpolate(sr.permute(0, 3, 1, 2), size=(H, Wd), mode='bilinear', align_corners=False)
        ref = ref_ohem_ce(upr, y, c[0], c[1], c[2], cws[k])
        (ref * float(g[k])).backward()
        assert abs(float(out[k, 0]) - float(ref.detach())) <= 2e-5 * abs(float(ref.detach())) + 1e-7, (k, out[k], ref)
        torch.testing.assert_close(d[k].cpu(), sr.grad, rtol=2e-4, atol=1e-7)


# --------------------------------------------------------------------------- #
# 5. neutral weights, entry points, validation
# --------------------------------------------------------------------------- #
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
        n, self.names = [x for x in self.names if 'ohem' in x], []
        return n


def test_neutral_weights_and_entry_points(be, monkeypatch):
    from led_net_amd import ops_train as T
    N, Hs, Ws, kept, thr, ignore = TF.CASES[0]
    s0, s1, y = TF._inputs(N, Hs, Ws, ignore, 11)
    H, Wd = 2 * Hs, 2 * Ws
    cfg = [(thr[0], kept[0], 1.0), (thr[1], kept[1], 0.4)]
    ones = W([1.0, 1.0])
    g = D(torch.tensor([1.0]))
    lg = D(F.interpolate(s0.permute(0, 3, 1, 2), size=(H, Wd), mode='bilinear', align_corners=False)
           .permute(0, 2, 3, 1).contiguous())
    spy = _Spy(monkeypatch)

    def rel(a, b):
        assert abs(float(a) - float(b)) <= 2e-6 * abs(float(b)) + 1e-8, (float(a), float(b))

    # generic
    o, w = T.ohem_ce_fwd(lg, D(y), *cfg[0], 255)
    dl = T.ohem_ce_bwd(lg, D(y), w, o, g, 1.0, 255)
    assert spy.take() == ['ledn_ohem_ce_fwd', 'ledn_ohem_ce_bwd']
    o1, w1 = T.ohem_ce_fwd(lg, D(y), *cfg[0], 255, class_weight=ones)
    dl1 = T.ohem_ce_bwd(lg, D(y), w1, o1, g, 1.0, 255, class_weight=ones)
    assert spy.take() == ['ledn_ohem_ce_w_fwd', 'ledn_ohem_ce_w_bwd']
    rel(o1[0], o[0])
    assert torch.equal(o1.cpu()[1:], o.cpu()[1:])
    torch.testing.assert_close(dl1.cpu(), dl.cpu(), rtol=2e-6, atol=1e-10)
    # resize-folded
    o, w = T.ohem_ce_up_fwd(D(s0), D(y), *cfg[0], 255)
    d = T.ohem_ce_up_bwd(D(s0), D(y), w, o, g, 1.0, 255)
    assert spy.take() == ['ledn_ohem_ce_up_fwd', 'ledn_ohem_ce_up_bwd']
    o1, w1 = T.ohem_ce_up_fwd(D(s0), D(y), *cfg[0], 255, class_weight=ones)
    d1 = T.ohem_ce_up_bwd(D(s0), D(y), w1, o1, g, 1.0, 255, class_weight=ones)
    assert spy.take() == ['ledn_ohem_ce_up_w_fwd', 'ledn_ohem_ce_up_w_bwd']
    rel(o1[0], o[0])
    assert torch.equal(o1.cpu()[1:], o.cpu()[1:])
    torch.testing.assert_close(d1.cpu(), d.cpu(), rtol=2e-6, atol=1e-10)
    # pair: positional call as before, explicit (None, None), then neutral weights
    o, w = T.ohem2_up_fwd(D(s0), D(s1), D(y), cfg[0], cfg[1], 255)
    da = T.ohem2_up_bwd(D(s0), D(s1), (H, Wd), w, o, g, g, 1.0, 0.4, 255)
    assert spy.take() == ['ledn_ohem2_up_fwd', 'ledn_ohem2_up_bwd']
    T.ohem2_up_fwd(D(s0), D(s1), D(y), cfg[0], cfg[1], 255, class_weights=(None, None))
    assert spy.take() == ['ledn_ohem2_up_fwd']
    o1, w1 = T.ohem2_up_fwd(D(s0), D(s1), D(y), cfg[0], cfg[1], 255, class_weights=(ones, ones))
    db = T.ohem2_up_bwd(D(s0), D(s1), (H, Wd), w1, o1, g, g, 1.0, 0.4, 255, class_weights=(ones, ones))
    assert spy.take() == ['ledn_ohem2_up_w_fwd', 'ledn_ohem2_up_w_bwd']
    for k in range(2):
        rel(o1[k, 0], o[k, 0])
        torch.testing.assert_close(db[k].cpu(), da[k].cpu(), rtol=2e-6, atol=1e-10)
    assert torch.equal(o1.cpu()[:, 1:], o.cpu()[:, 1:])


def test_class_weight_validation(be):
    from led_net_amd import ops_train as T
    from led_net_amd.ops import LednError
    s0, s1, y = TF._inputs(1, 4, 4, 'none', 3)
    lg = D(torch.randn(1, 8, 8, 5))
    y5 = D(torch.randint(0, 5, (1, 8, 8)))
    bad = [W([1.0, 2.0, 3.0]),                                         # wrong length
           D(torch.tensor([1.0, 2.0], dtype=torch.float64)),           # wrong dtype
           W([1.0, float('nan')]), W([float('inf'), 1.0]),            # not finite
           D(torch.ones(1, 2)),                                        # not a vector
           [1.0, 2.0]]                                                 # not a tensor
    for cw in bad:
        with pytest.raises(LednError):
            T.ohem_ce_up_fwd(D(s0), D(y), 0.9, 10, 1.0, 255, class_weight=cw)
        with pytest.raises(LednError):
            T.ohem2_up_fwd(D(s0), D(s1), D(y), (0.9, 10, 1.0), (0.9, 10, 1.0), 255, class_weights=(None, cw))
    with pytest.raises(LednError):
        T.ohem_ce_fwd(lg, y5, 0.9, 10, 1.0, 255, class_weight=W([1.0, 2.0]))       # 2 weights, 5 classes
    if _DEV[0].type == 'cuda':
        with pytest.raises(LednError):                                 # on another device than the logits
            T.ohem_ce_up_fwd(D(s0), D(y), 0.9, 10, 1.0, 255, class_weight=torch.ones(2))


# --------------------------------------------------------------------------- #
# 6. module and head
# --------------------------------------------------------------------------- #
def test_module_builds_and_keeps_the_reference_state_dict():
    import led_net_amd as L
    m = L.MODELS.build(dict(type='OhemCrossEntropy', thres=0.9, min_kept=100, class_weight=[0.8, 1.2]))
    assert m.class_weight == [0.8, 1.2] and list(m.state_dict()) == []
    assert L.MODELS.build(dict(type='OhemCrossEntropy')).class_weight is None
    assert L.MODELS.build(dict(type='OhemCrossEntropy', class_weight=(0.5, 2))).class_weight == (0.5, 2)
    for bad in ('weights.txt', [], [1.0, float('nan')], 3.0):
        with pytest.raises((TypeError, ValueError)):
            L.MODELS.build(dict(type='OhemCrossEntropy', class_weight=bad))
    cfg = L.load_config(CFG)['model']['decode_head']
    plain = L.MODELS.build(cfg)
    for c in cfg['loss_decode']:
        c['class_weight'] = [0.8, 1.2]
    weighted = L.MODELS.build(cfg)
    assert set(weighted.state_dict()) == set(plain.state_dict())
    assert [l.class_weight for l in weighted.loss_decode] == [[0.8, 1.2], [0.8, 1.2]]
    moved = weighted.to(torch.float64)                # .to() reaches the weight buffer like any other buffer
    assert moved.loss_decode[0]._class_weight.dtype == torch.float64


def test_module_forward_matches_the_reference_statements(be):
    import led_net_amd as L
    fx = Fixture('g21_ohemcw_c5')
    kw = fx.meta['kwargs']
    crit = L.MODELS.build(dict(type='OhemCrossEntropy', **kw)).to(_DEV[0])
    score = nhwc(fx.ins['score']).requires_grad_(True)
    loss = crit(score.permute(0, 3, 1, 2), D(fx.ins['target']))
    close(loss, fx.outs['loss'].reshape(()), 1e-4, 1e-6, 'module loss')
    loss.backward()
    close(nchw(score.grad), fx.gin['score'], 1e-3, 1e-8, 'module dscore')
    wrong = L.MODELS.build(dict(type='OhemCrossEntropy', class_weight=[1.0, 2.0])).to(_DEV[0])
    with pytest.raises(ValueError, match='class_weight has 2 entries'):
        wrong(score.permute(0, 3, 1, 2), D(fx.ins['target']))


HEAD_CASES = [  # label size, FUSE_LOSS_PAIR, (weights of loss 0, of loss 1) -> dispatch branch
    ((32, 40), 1, ([0.7, 1.6], [1.3, 0.5])),          # even, W % 4 == 0: the fused pair
    ((32, 40), 1, (None, [1.3, 0.5])),                # the pair with one unweighted loss
    ((32, 40), 0, ([0.7, 1.6], [1.3, 0.5])),          # two single resize-folded losses
    ((30, 38), 1, ([0.7, 1.6], None)),                # even, W % 4 != 0: single resize-folded losses
    ((31, 37), 1, ([0.7, 1.6], [1.3, 0.5])),          # odd: generic kernel on the resized logits
]


@pytest.mark.parametrize('hw,pair,cws', HEAD_CASES)
def test_led_head_loss_by_feat_with_class_weight(be, monkeypatch, hw, pair, cws):
    """LEDHead.loss_by_feat on seeded training logits vs oracle.spec.fuse_loss + the reference's weighted statements:
    losses, accuracy and the gradients of the four logit maps"""
    import led_net_amd as L
    from led_net_amd import train as TR
    monkeypatch.setattr(TR, 'FUSE_LOSS_PAIR', pair)
    H, Wd = hw
    cfg = L.load_config(CFG)['model']['decode_head']
    lcfg = [(0.9, 300, 1.0), (0.8, 5000, 0.4)]
    for c, (t, k, lw), cw in zip(cfg['loss_decode'], lcfg, cws):
        c.update(thres=t, min_kept=k, loss_weight=lw)
        if cw is not None:
            c['class_weight'] = cw
    head = L.MODELS.build(cfg).to(_DEV[0]).train()
    g = torch.Generator().manual_seed(H * 100 + Wd)
    h8, w8 = -(-H // 8), -(-Wd // 8)
    shapes = [(2, 2, h8, w8), (2, 2, h8, w8), (2, 2, H // 2, Wd // 2), (2, 2, H // 4, Wd // 4)]     # xc, xs, h1, h2
    ref_in = [(1.5 * torch.randn(s, generator=g)).requires_grad_(True) for s in shapes]
    label = torch.randint(0, 2, (2, 1, H, Wd), generator=g)
    label[:, :, :3] = 255
    ins = [nhwc(t).requires_grad_(True) for t in ref_in]
    samples = [L.SegDataSample(gt=D(label[i])) for i in range(2)]
    out = head.loss_by_feat(tuple(t.permute(0, 3, 1, 2) for t in ins), samples)
    (out['loss_context'] + 0.5 * out['loss_spatial']).backward()
    xc, xs, h1, h2 = ref_in
    y = label.squeeze(1)
    ctx, spa = spec.fuse_loss(xc, h1, h2, (H, Wd)), spec.fuse_loss(xs, h1, h2, (H, Wd))
    want0 = ref_ohem_ce(ctx, y, *lcfg[0], cws[0])
    want1 = ref_ohem_ce(spa, y, *lcfg[1], cws[1])
    (want0 + 0.5 * want1).backward()
    print('loss_context', float(out['loss_context']), float(want0), 'loss_spatial', float(out['loss_spatial']), float(want1))
    close(out['loss_context'].reshape(()), want0.detach(), 2e-5, 1e-7, 'loss_context')
    close(out['loss_spatial'].reshape(()), want1.detach(), 2e-5, 1e-7, 'loss_spatial')
    close(out['acc_seg'].reshape(-1), spec.accuracy(ctx.detach(), y, 255).reshape(-1), 1e-5, 1e-4, 'acc_seg')
    for name, t, r in zip(('xc', 'xs', 'h1', 'h2'), ins, ref_in):
        close(nchw(t.grad), r.grad, 2e-4, 1e-7, 'd/d' + name)


def test_head_rejects_a_weight_list_of_the_wrong_length(be):
    import led_net_amd as L
    cfg = L.load_config(CFG)['model']['decode_head']
    cfg['loss_decode'][1]['class_weight'] = [1.0, 1.0, 1.0]
    head = L.MODELS.build(cfg).to(_DEV[0]).train()
    ins = [D(torch.randn(s)) for s in ((1, 4, 4, 2), (1, 4, 4, 2), (1, 16, 16, 2), (1, 8, 8, 2))]
    samples = [L.SegDataSample(gt=D(torch.zeros(1, 32, 32, dtype=torch.int64)))]
    with pytest.raises(ValueError, match='class_weight has 3 entries but the logits have 2 classes'):
        head.loss_by_feat(tuple(t.permute(0, 3, 1, 2) for t in ins), samples)


# --------------------------------------------------------------------------- #
# 7. whole step: eager = captured replay and run = run, bit for bit (as tests/test_deterministic.py for the
# unweighted step)
# --------------------------------------------------------------------------- #
def _weighted_steps(dev, steps, graph):
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(CFG)
    for c, cw in zip(cfg['model']['decode_head']['loss_decode'], ([0.8, 1.2], [1.5, 0.6])):
        c['min_kept'] = 20000
        c['class_weight'] = cw
    model = L.MODELS.build(cfg['model'])
    model.set_act_dtype(torch.bfloat16)
    model.to(dev)
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (2, 3, 320, 320), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 2, (2, 1, 320, 320), dtype=torch.int64, generator=g)
    lab[:, :, :5, :] = 255
    samples = [L.SegDataSample(gt=lab[i].to(dev)) for i in range(2)]
    L.set_deterministic(True)
    try:
        tr = L.Trainer(model, cfg, max_iters=1000)
        losses = []
        if graph:
            tr.capture(img, samples, warmup=2, restore=True)
            for _ in range(steps):
                losses.append({k: v.detach().clone() for k, v in tr.replay(img, samples).items()})
        else:
            snap = ([p.detach().clone() for p in tr.params], [b.detach().clone() for b in model.buffers()], tr.iter)
            for _ in range(2):
                tr.train_step(img, samples)
            with torch.no_grad():
                for p, v in zip(tr.params, snap[0]):
                    p.copy_(v)
                for b, v in zip(model.buffers(), snap[1]):
                    b.copy_(v)
                tr.flat_mom.zero_()
            tr.iter = snap[2]
            for _ in range(steps):
                losses.append({k: v.detach().clone() for k, v in tr.train_step(img, samples).items()})
        if dev.type == 'cuda':
            torch.cuda.synchronize()
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, tr.flat_mom.clone()
    finally:
        L.set_deterministic(False)


def _bit_equal(a, b, what):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        for k in x:
            assert torch.equal(x[k], y[k]), f'{what}: step {i} {k}: {x[k].item()!r} vs {y[k].item()!r}'
    bad = [k for k in a[1] if not torch.equal(a[1][k], b[1][k])]
    assert not bad, f'{what}: {len(bad)} of {len(a[1])} tensors differ, e.g. {bad[:5]}'
    assert torch.equal(a[2], b[2]), f'{what}: momentum buffers differ'


@pytest.mark.gpu
def test_weighted_step_eager_equals_replay_and_repeats_bit_exactly():
    dev = torch.device('cuda:0')
    a = _weighted_steps(dev, 3, graph=False)
    b = _weighted_steps(dev, 3, graph=False)
    _bit_equal(a, b, 'two deterministic eager runs of the weighted step')
    c = _weighted_steps(dev, 3, graph=True)
    _bit_equal(a, c, 'weighted step: hipGraph replay vs eager')
    import math
    assert all(math.isfinite(float(v)) for d in a[0] for v in d.values())


def test_weighted_step_repeats_bit_exactly_on_the_emulator(emu):
    slow_on_emu(torch.device('cpu'))
    dev = torch.device('cpu')
    _bit_equal(_weighted_steps(dev, 1, graph=False), _weighted_steps(dev, 1, graph=False), 'two emulator runs')


# --------------------------------------------------------------------------- #
# 8. the training CLI
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
def test_train_cli_takes_class_weight_from_cfg_options(tmp_path):
    def run(extra, wd):
        env = dict(os.environ, PYTHONPATH=ROOT, LEDN_DETERMINISTIC='1')
        args = [sys.executable, 'tools/train.py', CFG, '--max-iters', '3', '--batch-size', '2', '--height', '320',
                '--width', '320', '--f32', '--work-dir', str(tmp_path / wd)] + extra
        r = subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, f'{args}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
        m = re.search(r'\[\s*3/3\].*loss_context: ([0-9.eE+-]+).*loss_spatial: ([0-9.eE+-]+)', r.stdout)
        assert m, r.stdout[-2000:]
        assert 'hipGraph replay' in r.stdout
        return float(m.group(1)), float(m.group(2))

    plain = run([], 'plain')
    again = run([], 'again')
    weighted = run(['--cfg-options', 'model.decode_head.loss_decode.0.class_weight=[0.8,1.2]'], 'weighted')
    print('loss_context / loss_spatial after 3 iterations: unweighted', plain, 'again', again, 'weighted', weighted)
    assert plain == again                                  # deterministic mode: the unweighted run repeats
    assert weighted[0] != plain[0]
