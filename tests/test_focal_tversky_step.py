"""The whole training step with LEDHead(loss_decode=[FocalLoss, TverskyLoss]) (tests/data/lednet_focal_tversky_config.py):
deterministic eager runs repeat bit for bit and equal the hipGraph replay (the step holds no host read-back: Focal's
divisor is a host constant, Tversky's per-(image, class) terms and backward coefficients are formed on the device), one
f32 step against the oracle model plus the restated reference losses, and the training CLI."""
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
from test_focal_tversky import FT_CFG, ROOT, ref_focal, ref_tversky


def ft_steps(dev, steps, graph):
    """as test_seg_losses_step._steps (2 x 3 x 320 x 320, bf16, deterministic mode), on the Focal + Tversky config"""
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(FT_CFG)
    model = L.MODELS.build(cfg['model'])
    assert [type(m).__name__ for m in model.decode_head.loss_decode] == ['FocalLoss', 'TverskyLoss']
    model.set_act_dtype(torch.bfloat16)
    model.to(dev)
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (2, 3, 320, 320), dtype=torch.uint8, generator=g).to(dev)
    lab = (torch.rand((2, 1, 320, 320), generator=g) < 0.1).long()
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


@pytest.mark.gpu
def test_focal_tversky_step_eager_equals_replay_and_repeats_bit_exactly():
    dev = torch.device('cuda:0')
    a = ft_steps(dev, 3, graph=False)
    b = ft_steps(dev, 3, graph=False)
    SS._bit_equal(a, b, 'two deterministic eager runs of the Focal + Tversky step')
    c = ft_steps(dev, 3, graph=True)
    SS._bit_equal(a, c, 'Focal + Tversky step: hipGraph replay vs eager')
    print([{k: float(v.reshape(-1)[0]) for k, v in d.items()} for d in a[0]])
    assert all(math.isfinite(float(v)) for d in a[0] for v in d.values())
    assert all(set(d) == {'decode.loss_context', 'decode.loss_spatial', 'decode.acc_seg'} for d in a[0])


def test_focal_tversky_step_repeats_bit_exactly_on_the_emulator(emu):
    slow_on_emu(torch.device('cpu'))
    dev = torch.device('cpu')
    SS._bit_equal(ft_steps(dev, 1, graph=False), ft_steps(dev, 1, graph=False), 'two emulator runs')


def _f32_step(dev):
    """one f32 step: the losses of mode='loss' and a sample of parameter gradients against oracle.spec's network and
    fusion pyramid with the restated FocalLoss / TverskyLoss(loss_weight=0.4) on top, under torch autograd"""
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(FT_CFG)
    model = L.MODELS.build(cfg['model'])
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (2, 3, 320, 320), dtype=torch.uint8, generator=g)
    lab = (torch.rand((2, 1, 320, 320), generator=g) < 0.1).long()
    lab[:, :, :6, :] = 255
    lab[:, :, :, -5:] = 255
    names = [k for k in sd if k.startswith('decode_head.') and k.endswith(('.1.weight', '.1.bias'))]   # the last convs
    assert len(names) >= 4, names
    leaf = {k: sd[k].clone().requires_grad_(True) for k in names}
    sdr = dict(sd, **leaf)
    feats = spec.lednet(spec.preprocess(img), sdr, training=True, p='backbone.')
    xc, xs, h1, h2 = spec.led_head(feats, sdr, 'decode_head.', True)
    y = lab.squeeze(1)
    ctx, spa = spec.fuse_loss(xc, h1, h2, y.shape[1:]), spec.fuse_loss(xs, h1, h2, y.shape[1:])
    want = {'decode.loss_context': ref_focal(ctx, y, gamma=2.0, alpha=0.5, loss_weight=1.0, ignore_index=255),
            'decode.loss_spatial': ref_tversky(spa, y, alpha=0.3, beta=0.7, loss_weight=0.4),
            'decode.acc_seg': spec.accuracy(ctx.detach(), y, 255)}
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
    return got, want, grads, leaf


def _check_f32_step(dev):
    got, want, grads, leaf = _f32_step(dev)
    # acc_seg is a count: the whole-step bound of test_train.py (2e-3 / 1e-4), as in test_seg_losses_step.py
    bounds = (('decode.loss_context', (2e-5, 1e-7)), ('decode.loss_spatial', (2e-5, 1e-7)), ('decode.acc_seg', (2e-3, 1e-4)))
    for k, _ in bounds:
        print(k, float(got[k].detach().reshape(-1)[0]), float(want[k].detach().reshape(-1)[0]))
    for k, (rt, at) in bounds:
        torch.testing.assert_close(got[k].detach().reshape(-1).float().cpu(), want[k].detach().reshape(-1), rtol=rt, atol=at,
                                   msg=lambda m: f'{k}: {m}')
    # the gradients of the heads' last convolutions: sums over the pixels of (loss gradient x head feature).  The loss
    # gradients are held to 2e-4 elementwise at the head level (test_focal_tversky.py) and the features carry the f32
    # error of the network in front of the head, for which test_train.py's whole-step bound is 2e-3: that bound, on the
    # relative L2 error of each tensor
    gmax = max(float(leaf[k].grad.norm()) for k in grads)
    assert gmax > 0
    for k, gk in grads.items():
        rel = float((gk - leaf[k].grad).norm()) / max(float(leaf[k].grad.norm()), 1e-4 * gmax)
        print(f'{k}: |grad| {float(leaf[k].grad.norm()):.3e} rel-L2 error {rel:.2e}')
        assert rel <= 2e-3, (k, rel)


def test_focal_tversky_f32_step_vs_oracle_model(emu):
    _check_f32_step(torch.device('cpu'))


@pytest.mark.gpu
def test_train_cli_runs_the_focal_tversky_config(tmp_path):
    def run(env_extra, wd):
        env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
        args = [sys.executable, 'tools/train.py', FT_CFG, '--max-iters', '3', '--batch-size', '2', '--height', '320',
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
    import led_net_amd as L
    ckpt = tmp_path / 'det' / 'iter_3.pth'
    assert ckpt.is_file(), os.listdir(tmp_path / 'det')
    model = L.MODELS.build(L.load_config(FT_CFG)['model'])
    meta = L.load_checkpoint(model, str(ckpt), strict=True)['meta']
    assert meta['iter'] == 3
