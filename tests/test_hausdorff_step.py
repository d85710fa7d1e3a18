"""The whole training step with LEDHead(loss_decode=[CrossEntropyLoss, HuasdorffDisstanceLoss])
(tests/data/lednet_hausdorff_config.py): deterministic eager runs repeat bit for bit and equal the hipGraph replay (the
distance transform runs on the device with a launch sequence that depends on the sizes only: no host read-back inside
the step), the Hausdorff kernels give the same bits whatever the library's deterministic switch says (they have no
atomics at all), one f32 step against the oracle model with the restated losses on top, and the training CLI.

The f32 step and the argmax mask.  The loss is not continuous in the logits: a pixel whose two logits lie closer than
the network's own f32 error may fall on either side of the prediction mask, and the distance map around it moves with
it.  The squared distance transform is monotone in the mask (more foreground: no distance shrinks) and every term
D * delta is non-negative, so the restated loss with every such pixel (|l_1 - l_0| < TIE, the margin of smoke()'s argmax
check) counted as background / as foreground brackets the loss of ANY assignment of them: the step's loss must lie in
that bracket, widened by the whole-step bound of test_train.py, 2e-3 / 1e-4 (the kernels' own 1e-4 / 1e-6 is held in
test_hausdorff.py; here the logits are the f32 network's, up to 28 in size at the initial weights, and the labels are
filled shapes, so the network's logit error does not average out over the pixels as it does on the random labels
that test_seg_losses_step.py's 2e-5 was set on -- the CrossEntropyLoss term missed that bound with 3.3e-5 on these
labels on the emulator (1.0e-5 on the device), and takes the whole-step bound too).  The parameter gradients are linear
in D; the step's D differs from the oracle's only where the two bracketing maps differ, by at most their difference, so
the relative L2 distance of the two bracketing gradients is added to the project's whole-step bound 2e-3."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import slow_on_emu
from oracle import spec
import test_seg_losses_step as SS
from test_seg_losses import ref_ce
from test_hausdorff import HD_CFG, ROOT, blob_case, ref_hausdorff, sep_edt_sq

TIE = 1e-3


def _labels(g):
    """2 x 1 x 320 x 320: two filled rectangles and a disc per image, a band of 255 at the top"""
    yy, xx = torch.meshgrid(torch.arange(320), torch.arange(320), indexing='ij')
    lab = torch.zeros((2, 1, 320, 320), dtype=torch.int64)
    lab[0, 0, 40:200, 60:250] = 1
    lab[0, 0, 230:300, 20:90] = 1
    lab[1, 0, 100:300, 30:130] = 1
    lab[1, 0][(yy - 120) ** 2 + (xx - 230) ** 2 <= 60 ** 2] = 1
    lab[:, :, :int(torch.randint(4, 8, (1,), generator=g)), :] = 255
    return lab


def hd_steps(dev, steps, graph):
    """as test_seg_losses_step._steps (2 x 3 x 320 x 320, bf16, deterministic mode), on the CE + Hausdorff config"""
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(HD_CFG)
    model = L.MODELS.build(cfg['model'])
    assert [type(m).__name__ for m in model.decode_head.loss_decode] == ['CrossEntropyLoss', 'HuasdorffDisstanceLoss']
    model.set_act_dtype(torch.bfloat16)
    model.to(dev)
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (2, 3, 320, 320), dtype=torch.uint8, generator=g).to(dev)
    lab = _labels(g)
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


@pytest.mark.gpu
def test_hausdorff_step_eager_equals_replay_and_repeats_bit_exactly():
    dev = torch.device('cuda:0')
    a = hd_steps(dev, 3, graph=False)
    b = hd_steps(dev, 3, graph=False)
    SS._bit_equal(a, b, 'two deterministic eager runs of the CE + Hausdorff step')
    c = hd_steps(dev, 3, graph=True)
    SS._bit_equal(a, c, 'CE + Hausdorff step: hipGraph replay vs eager')
    print([{k: float(v.reshape(-1)[0]) for k, v in d.items()} for d in a[0]])
    assert all(math.isfinite(float(v)) for d in a[0] for v in d.values())
    assert all(set(d) == {'decode.loss_context', 'decode.loss_spatial', 'decode.acc_seg'} for d in a[0])


def _hausdorff_bits(dev):
    from led_net_amd import ops_train as T
    x, y = blob_case(2, 2, 127, 161, 8)
    lg, yd = x.permute(0, 2, 3, 1).contiguous().to(dev), y.to(dev)
    out, work = T.hausdorff_loss_fwd(lg, yd, loss_weight=0.4)
    return out.clone(), T.hausdorff_loss_bwd(lg, yd, work, out, torch.ones(1, device=dev)), work[4:4 + y.numel()].clone()


def _check_mode_independent(dev):
    import led_net_amd as L
    a = _hausdorff_bits(dev)
    L.set_deterministic(True)
    try:
        b = _hausdorff_bits(dev)
    finally:
        L.set_deterministic(False)
    c = _hausdorff_bits(dev)
    for u, v in ((a, b), (a, c)):
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(u, v))
    assert float(a[0][0]) > 0 and bool(torch.isfinite(a[1]).all())


def test_hausdorff_kernels_give_the_same_bits_in_default_and_deterministic_mode(emu):
    _check_mode_independent(torch.device('cpu'))


@pytest.mark.gpu
def test_hausdorff_kernels_give_the_same_bits_in_default_and_deterministic_mode_gpu():
    _check_mode_independent(torch.device('cuda:0'))


def test_hausdorff_step_repeats_bit_exactly_on_the_emulator(emu):
    slow_on_emu(torch.device('cpu'))
    dev = torch.device('cpu')
    SS._bit_equal(hd_steps(dev, 1, graph=False), hd_steps(dev, 1, graph=False), 'two emulator runs')


def _f32_step(dev):
    """one f32 step: the losses of mode='loss' and a sample of parameter gradients against oracle.spec's network and
    fusion pyramid with the restated CrossEntropyLoss(avg_non_ignore) / HuasdorffDisstanceLoss on top, under torch
    autograd; the Hausdorff restatement three times: with the oracle's own argmax mask, and with the pixels inside TIE
    counted as background / as foreground (the module docstring)"""
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(HD_CFG)
    lw = cfg['model']['decode_head']['loss_decode'][1]['loss_weight']
    model = L.MODELS.build(cfg['model'])
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (2, 3, 320, 320), dtype=torch.uint8, generator=g)
    lab = _labels(g)
    lab[:, :, :, -5:] = 255
    names = [k for k in sd if k.startswith('decode_head.') and k.endswith(('.1.weight', '.1.bias'))]   # the last convs
    assert len(names) >= 4, names
    leaf = {k: sd[k].clone().requires_grad_(True) for k in names}
    sdr = dict(sd, **leaf)
    feats = spec.lednet(spec.preprocess(img), sdr, training=True, p='backbone.')
    xc, xs, h1, h2 = spec.led_head(feats, sdr, 'decode_head.', True)
    y = lab.squeeze(1)
    ctx, spa = spec.fuse_loss(xc, h1, h2, y.shape[1:]), spec.fuse_loss(xs, h1, h2, y.shape[1:])
    diff = (spa[:, 1] - spa[:, 0]).detach()
    masks = {'mid': (diff > 0).long(), 'lo': (diff >= TIE).long(), 'hi': (diff > -TIE).long()}
    print('pixels inside the tie margin:', int((diff.abs() < TIE).sum()), 'of', diff.numel(),
          'predicted foreground:', float(masks['mid'].float().mean()))
    hd = {k: ref_hausdorff(spa.double(), y, loss_weight=lw, edt=sep_edt_sq, seg_mask=m).float() for k, m in masks.items()}
    want = {'decode.loss_context': ref_ce(ctx, y, avg_non_ignore=True, loss_weight=1.0, ignore_index=255),
            'decode.loss_spatial': hd['mid'], 'decode.acc_seg': spec.accuracy(ctx.detach(), y, 255)}
    ends = {}
    for k in ('lo', 'hi'):
        gs = torch.autograd.grad(hd[k], [leaf[n] for n in names], retain_graph=True, allow_unused=True)
        ends[k] = {n: (torch.zeros_like(leaf[n]) if v is None else v) for n, v in zip(names, gs)}
    (want['decode.loss_context'] + want['decode.loss_spatial']).backward()
    model.to(dev)
    tr = L.Trainer(model, cfg, max_iters=80000)
    samples = [L.SegDataSample(gt=lab[i].to(dev)) for i in range(2)]
    got = tr.train_step(img.to(dev), samples)            # (the losses of the initial weights; attaches the gradient views)
    model.load_state_dict(sd)                            # the step moved the weights: back to the oracle's
    tr.forward_backward(img.to(dev), samples)
    by_name = dict(model.named_parameters())
    grads = {}
    for k in names:
        i = [j for j, q in enumerate(tr.params) if q is by_name[k]]
        assert len(i) == 1, k
        grads[k] = tr.views[i[0]].detach().cpu().clone()
    return got, want, grads, leaf, hd, ends


def _check_f32_step(dev):
    got, want, grads, leaf, hd, ends = _f32_step(dev)
    for k in ('decode.loss_context', 'decode.loss_spatial', 'decode.acc_seg'):
        print(k, float(got[k].detach().reshape(-1)[0]), float(want[k].detach().reshape(-1)[0]))
    lo, hi = float(hd['lo'].detach()), float(hd['hi'].detach())
    print('Hausdorff bracket', lo, hi, 'CE', float(want['decode.loss_context'].detach()))
    # the whole-step bound of test_train.py (2e-3 / 1e-4), for the CE, the count acc_seg and around the bracket
    for k, (rt, at) in (('decode.loss_context', (2e-3, 1e-4)), ('decode.acc_seg', (2e-3, 1e-4))):
        torch.testing.assert_close(got[k].detach().reshape(-1).float().cpu(), want[k].detach().reshape(-1), rtol=rt, atol=at,
                                   msg=lambda m: f'{k}: {m}')
    sp = float(got['decode.loss_spatial'].detach().reshape(-1)[0])
    assert lo <= float(want['decode.loss_spatial'].detach()) <= hi
    assert lo - (2e-3 * lo + 1e-4) <= sp <= hi + (2e-3 * hi + 1e-4), (lo, sp, hi)
    # the two terms of this config are of the same order (the comment of lednet_hausdorff_config.py)
    assert 0.1 <= sp / float(got['decode.loss_context'].detach().reshape(-1)[0]) <= 10
    # the gradients of the heads' last convolutions, relative L2 error per tensor: test_train.py's whole-step bound
    # plus the relative distance of the two bracketing gradients
    gmax = max(float(leaf[k].grad.norm()) for k in grads)
    assert gmax > 0
    for k, gk in grads.items():
        den = max(float(leaf[k].grad.norm()), 1e-4 * gmax)
        rel = float((gk - leaf[k].grad).norm()) / den
        slack = float((ends['hi'][k] - ends['lo'][k]).norm()) / den
        print(f'{k}: |grad| {float(leaf[k].grad.norm()):.3e} rel-L2 error {rel:.2e} (bracket {slack:.2e})')
        assert rel <= 2e-3 + slack, (k, rel, slack)


def test_hausdorff_f32_step_vs_oracle_model(emu):
    slow_on_emu(torch.device('cpu'))
    _check_f32_step(torch.device('cpu'))


@pytest.mark.gpu
def test_hausdorff_f32_step_vs_oracle_model_gpu():
    _check_f32_step(torch.device('cuda:0'))


@pytest.mark.gpu
def test_train_cli_runs_the_hausdorff_config(tmp_path):
    def run(env_extra, wd):
        env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
        args = [sys.executable, 'tools/train.py', HD_CFG, '--max-iters', '3', '--batch-size', '2', '--height', '320',
                '--width', '320', '--f32', '--work-dir', str(tmp_path / wd)]
        r = subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, f'{args}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
        m = re.search(r'\[\s*3/3\].*loss_context: ([0-9.eE+-]+).*loss_spatial: ([0-9.eE+-]+)', r.stdout)
        assert m, r.stdout[-2000:]
        assert 'hipGraph replay' in r.stdout
        return float(m.group(1)), float(m.group(2))

    det = run({'LEDN_DETERMINISTIC': '1'}, 'det')
    again = run({'LEDN_DETERMINISTIC': '1'}, 'again')
    print('loss_context / loss_spatial after 3 iterations:', det, again)
    assert all(math.isfinite(v) for v in det)
    assert det == again
