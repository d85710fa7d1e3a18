"""The whole training step with LEDHead(loss_decode=[CrossEntropyLoss, LovaszLoss]) (tests/data/lednet_lovasz_config.py):
deterministic eager runs repeat bit for bit and equal the hipGraph replay (the sort has a fixed length and the counts
it needs stay on the device: no host read-back inside the step), the Lovasz kernels give the same bits whatever the
library's deterministic switch says (they have no float atomics to switch off), one f32 step against the oracle model
with the restated losses on top, and the training CLI."""
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
from test_lovasz import LV_CFG, ROOT, gridded_case, ref_lovasz


def lv_steps(dev, steps, graph):
    """as test_seg_losses_step._steps (2 x 3 x 320 x 320, bf16, deterministic mode), on the CE + Lovasz config"""
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(LV_CFG)
    model = L.MODELS.build(cfg['model'])
    assert [type(m).__name__ for m in model.decode_head.loss_decode] == ['CrossEntropyLoss', 'LovaszLoss']
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
def test_lovasz_step_eager_equals_replay_and_repeats_bit_exactly():
    dev = torch.device('cuda:0')
    a = lv_steps(dev, 3, graph=False)
    b = lv_steps(dev, 3, graph=False)
    SS._bit_equal(a, b, 'two deterministic eager runs of the CE + Lovasz step')
    c = lv_steps(dev, 3, graph=True)
    SS._bit_equal(a, c, 'CE + Lovasz step: hipGraph replay vs eager')
    print([{k: float(v.reshape(-1)[0]) for k, v in d.items()} for d in a[0]])
    assert all(math.isfinite(float(v)) for d in a[0] for v in d.values())
    assert all(set(d) == {'decode.loss_context', 'decode.loss_spatial', 'decode.acc_seg'} for d in a[0])


def _lovasz_bits(dev):
    from led_net_amd import ops_train as T
    x, y = gridded_case(2, 127, 161, 8)
    lg, yd = x.permute(0, 2, 3, 1).contiguous().to(dev), y.to(dev)
    out, work = T.lovasz_loss_fwd(lg, yd, per_image=True, class_weight=torch.tensor([0.7, 1.6], device=dev))
    return out.clone(), T.lovasz_loss_bwd(lg, yd, work, out, torch.ones(1, device=dev))


def _check_mode_independent(dev):
    import led_net_amd as L
    a = _lovasz_bits(dev)
    L.set_deterministic(True)
    try:
        b = _lovasz_bits(dev)
    finally:
        L.set_deterministic(False)
    c = _lovasz_bits(dev)
    for u, v in ((a, b), (a, c)):
        assert torch.equal(u[0], v[0]) and torch.equal(u[1], v[1])


def test_lovasz_kernels_give_the_same_bits_in_default_and_deterministic_mode(emu):
    _check_mode_independent(torch.device('cpu'))


@pytest.mark.gpu
def test_lovasz_kernels_give_the_same_bits_in_default_and_deterministic_mode_gpu():
    _check_mode_independent(torch.device('cuda:0'))


def test_lovasz_step_repeats_bit_exactly_on_the_emulator(emu):
    slow_on_emu(torch.device('cpu'))
    dev = torch.device('cpu')
    SS._bit_equal(lv_steps(dev, 1, graph=False), lv_steps(dev, 1, graph=False), 'two emulator runs')


def _f32_step(dev):
    """one f32 step: the losses of mode='loss' and a sample of parameter gradients against oracle.spec's network and
    fusion pyramid with the restated CrossEntropyLoss(avg_non_ignore) / LovaszLoss(loss_weight=0.4) on top, under torch
    autograd.  The Lovasz restatement runs on the f64 copy of the oracle's spatial logits (the reference's own f32
    Lovasz gradient is off by up to 1e-3 of its largest entry at this size, the issue's table)"""
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(LV_CFG)
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
    want = {'decode.loss_context': ref_ce(ctx, y, avg_non_ignore=True, loss_weight=1.0, ignore_index=255),
            'decode.loss_spatial': ref_lovasz(spa.double(), y, reduction='none', loss_weight=0.4).float(),
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
    # CE: the whole-step bound of test_seg_losses_step.py; Lovasz: the project's loss tolerance (test_lovasz.py) -- the
    # loss follows the network's f32 logit error through the ranking; acc_seg is a count (test_train.py's 2e-3 / 1e-4)
    bounds = (('decode.loss_context', (2e-5, 1e-7)), ('decode.loss_spatial', (1e-4, 1e-6)), ('decode.acc_seg', (2e-3, 1e-4)))
    for k, _ in bounds:
        print(k, float(got[k].detach().reshape(-1)[0]), float(want[k].detach().reshape(-1)[0]))
    for k, (rt, at) in bounds:
        torch.testing.assert_close(got[k].detach().reshape(-1).float().cpu(), want[k].detach().reshape(-1), rtol=rt, atol=at,
                                   msg=lambda m: f'{k}: {m}')
    # the gradients of the heads' last convolutions, relative L2 error per tensor: test_train.py's whole-step bound
    gmax = max(float(leaf[k].grad.norm()) for k in grads)
    assert gmax > 0
    for k, gk in grads.items():
        rel = float((gk - leaf[k].grad).norm()) / max(float(leaf[k].grad.norm()), 1e-4 * gmax)
        print(f'{k}: |grad| {float(leaf[k].grad.norm()):.3e} rel-L2 error {rel:.2e}')
        assert rel <= 2e-3, (k, rel)


def test_lovasz_f32_step_vs_oracle_model(emu):
    _check_f32_step(torch.device('cpu'))


@pytest.mark.gpu
def test_lovasz_f32_step_vs_oracle_model_gpu():
    _check_f32_step(torch.device('cuda:0'))


@pytest.mark.gpu
def test_train_cli_runs_the_lovasz_config(tmp_path):
    def run(env_extra, wd):
        env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
        args = [sys.executable, 'tools/train.py', LV_CFG, '--max-iters', '3', '--batch-size', '2', '--height', '320',
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
