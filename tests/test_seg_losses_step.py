"""The whole training step with LEDHead(loss_decode=[CrossEntropyLoss, DiceLoss]) (tests/data/lednet_ce_dice_config.py):
deterministic eager runs repeat bit for bit and equal the hipGraph replay (the step holds no host read-back: the
divisor and the per-image Dice terms are formed on the device), one f32 step against the oracle model plus the
reference's loss statements, and the training CLI."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import slow_on_emu
from oracle import spec
from test_seg_losses import CE_DICE_CFG, ROOT, ref_ce, ref_dice


def _steps(dev, steps, graph):
    """as test_ohem_class_weight._weighted_steps: 2 x 3 x 320 x 320, bf16, deterministic mode"""
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(CE_DICE_CFG)
    model = L.MODELS.build(cfg['model'])
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


def _bit_equal(a, b, what):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        for k in x:
            assert torch.equal(x[k], y[k]), f'{what}: step {i} {k}: {x[k].item()!r} vs {y[k].item()!r}'
    bad = [k for k in a[1] if not torch.equal(a[1][k], b[1][k])]
    assert not bad, f'{what}: {len(bad)} of {len(a[1])} tensors differ, e.g. {bad[:5]}'
    assert torch.equal(a[2], b[2]), f'{what}: momentum buffers differ'


@pytest.mark.gpu
def test_ce_dice_step_eager_equals_replay_and_repeats_bit_exactly():
    dev = torch.device('cuda:0')
    a = _steps(dev, 3, graph=False)
    b = _steps(dev, 3, graph=False)
    _bit_equal(a, b, 'two deterministic eager runs of the CE + Dice step')
    c = _steps(dev, 3, graph=True)
    _bit_equal(a, c, 'CE + Dice step: hipGraph replay vs eager')
    print([{k: float(v.reshape(-1)[0]) for k, v in d.items()} for d in a[0]])
    assert all(math.isfinite(float(v)) for d in a[0] for v in d.values())
    assert all(set(d) == {'decode.loss_context', 'decode.loss_spatial', 'decode.acc_seg'} for d in a[0])


def test_ce_dice_step_repeats_bit_exactly_on_the_emulator(emu):
    slow_on_emu(torch.device('cpu'))
    dev = torch.device('cpu')
    _bit_equal(_steps(dev, 1, graph=False), _steps(dev, 1, graph=False), 'two emulator runs')


def test_ce_dice_f32_step_vs_oracle_model(emu):
    """one f32 step on the emulator: the losses of mode='loss' against oracle.spec's network and fusion pyramid with the
    reference's CrossEntropyLoss(avg_non_ignore=True) / DiceLoss(loss_weight=0.4) statements on top (the head passes
    ignore_index=255 to the cross-entropy), the two losses at the head-level tolerances 2e-5 / 1e-7"""
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(CE_DICE_CFG)
    model = L.MODELS.build(cfg['model'])
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (2, 3, 320, 320), dtype=torch.uint8, generator=g)
    lab = (torch.rand((2, 1, 320, 320), generator=g) < 0.1).long()
    lab[:, :, :6, :] = 255
    lab[:, :, :, -5:] = 255
    with torch.no_grad():
        feats = spec.lednet(spec.preprocess(img), sd, training=True, p='backbone.')
        xc, xs, h1, h2 = spec.led_head(feats, sd, 'decode_head.', True)
        y = lab.squeeze(1)
        ctx, spa = spec.fuse_loss(xc, h1, h2, y.shape[1:]), spec.fuse_loss(xs, h1, h2, y.shape[1:])
        want = {'decode.loss_context': ref_ce(ctx, y, avg_non_ignore=True, loss_weight=1.0, ignore_index=255),
                'decode.loss_spatial': ref_dice(spa, y, loss_weight=0.4),
                'decode.acc_seg': spec.accuracy(ctx, y, 255)}
    tr = L.Trainer(model, cfg, max_iters=80000)
    got = tr.train_step(img, [L.SegDataSample(gt=lab[i]) for i in range(2)])
    # acc_seg is a count: a pixel whose two fused logits tie to within the f32 error of the NETWORK in front of the head
    # flips its argmax, which no loss kernel can change -- the whole-step bound of test_train.py (2e-3 / 1e-4) applies
    bounds = (('decode.loss_context', (2e-5, 1e-7)), ('decode.loss_spatial', (2e-5, 1e-7)), ('decode.acc_seg', (2e-3, 1e-4)))
    for k, _ in bounds:
        print(k, float(got[k].reshape(-1)[0]), float(want[k].reshape(-1)[0]))
    for k, (rt, at) in bounds:
        torch.testing.assert_close(got[k].detach().reshape(-1).float(), want[k].reshape(-1), rtol=rt, atol=at,
                                   msg=lambda m: f'{k}: {m}')


@pytest.mark.gpu
def test_train_cli_runs_the_ce_dice_config(tmp_path):
    def run(env_extra, wd):
        env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
        args = [sys.executable, 'tools/train.py', CE_DICE_CFG, '--max-iters', '3', '--batch-size', '2', '--height', '320',
                '--width', '320', '--f32', '--work-dir', str(tmp_path / wd)]
        r = subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, f'{args}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
        m = re.search(r'\[\s*3/3\].*loss_context: ([0-9.eE+-]+).*loss_spatial: ([0-9.eE+-]+)', r.stdout)
        assert m, r.stdout[-2000:]
        assert 'hipGraph replay' in r.stdout
        return float(m.group(1)), float(m.group(2))

    plain = run({}, 'plain')
    det = run({'LEDN_DETERMINISTIC': '1'}, 'det')
    again = run({'LEDN_DETERMINISTIC': '1'}, 'again')
    print('loss_context / loss_spatial after 3 iterations:', plain, det, again)
    assert all(math.isfinite(v) for v in plain + det)
    assert det == again
