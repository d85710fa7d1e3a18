"""The whole network with 19 classes (tests/data/lednet_c19_config.py: LEDHead's head_x1 / head_x2 are num_classes wide and
run on csrc/head_mc.hip in bf16): one f32 step against the oracle, deterministic bf16 steps eager / hipGraph, predict, and
the training CLI with --cfg-options model.decode_head.num_classes=19."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C19_CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_c19_config.py')
TWO_CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_test_config.py')


def _batch(seed, dev):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (2, 3, 320, 320), dtype=torch.uint8, generator=g)
    lab = torch.randint(0, 19, (2, 1, 320, 320), dtype=torch.int64, generator=g)
    lab[:, :, :6, :] = 255
    lab[:, :, :, -5:] = 255
    return img.to(dev), lab.to(dev)


def test_c19_f32_step_vs_oracle_model(emu):
    """one f32 step on the emulator, 2 x 3 x 320 x 320, labels in [0, 19) with an ignored border: the losses of mode='loss'
    against oracle.spec.loss on the model's own state dict, at the two-class whole-step bounds of tests/test_train.py
    (2e-3 / 1e-4).  The thresholds are not frozen through spec.TRACE (tests/test_train_frozen.py does that for its
    per-parameter gradient comparison; tests/test_train.py's loss comparison, whose bounds these are, does not)."""
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(C19_CFG)
    assert cfg['model']['decode_head']['num_classes'] == 19
    model = L.MODELS.build(cfg['model'])
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    assert tuple(sd['decode_head.head_x1.0.conv.weight'].shape) == (19, 32, 3, 3)
    img, lab = _batch(11, torch.device('cpu'))
    with torch.no_grad():
        want = spec.loss(spec.preprocess(img), lab, sd)
    tr = L.Trainer(model, cfg, max_iters=80000)
    got = tr.train_step(img, [L.SegDataSample(gt=lab[i]) for i in range(2)])
    keys = ('decode.loss_context', 'decode.loss_spatial', 'decode.acc_seg')
    for k in keys:
        print(k, float(got[k].reshape(-1)[0]), float(want[k].reshape(-1)[0]))
    for k in keys:
        torch.testing.assert_close(got[k].detach().reshape(-1).float(), want[k].detach().reshape(-1).float(), rtol=2e-3,
                                   atol=1e-4, msg=lambda m: f'{k}: {m}')


def _steps(dev, steps, graph):
    """as tests/test_seg_losses_step.py::_steps: 2 x 3 x 320 x 320, bf16, deterministic mode"""
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(C19_CFG)
    model = L.MODELS.build(cfg['model'])
    model.set_act_dtype(torch.bfloat16)
    model.to(dev)
    img, lab = _batch(5, dev)
    samples = [L.SegDataSample(gt=lab[i]) for i in range(2)]
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
def test_c19_step_eager_equals_replay_and_repeats_bit_exactly():
    dev = torch.device('cuda:0')
    a = _steps(dev, 3, graph=False)
    b = _steps(dev, 3, graph=False)
    _bit_equal(a, b, 'two deterministic eager runs of the 19-class step')
    c = _steps(dev, 3, graph=True)
    _bit_equal(a, c, '19-class step: hipGraph replay vs eager')
    print([{k: float(v.reshape(-1)[0]) for k, v in d.items()} for d in a[0]])
    assert all(math.isfinite(float(v)) for d in a[0] for v in d.values())
    assert all(set(d) == {'decode.loss_context', 'decode.loss_spatial', 'decode.acc_seg'} for d in a[0])


@pytest.mark.gpu
def test_c19_predict():
    import led_net_amd as L
    from led_net_amd import ops
    dev = torch.device('cuda:0')
    torch.manual_seed(304)
    cfg = L.load_config(C19_CFG)
    model = L.MODELS.build(cfg['model'])
    model.set_act_dtype(torch.bfloat16)
    model.to(dev).eval()
    img = torch.randint(0, 256, (1, 3, 320, 320), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():
        out = model(img, mode='predict')
    assert len(out) == 1
    logits, mask = out[0].seg_logits.data, out[0].pred_sem_seg.data
    assert tuple(logits.shape) == (19, 320, 320) and tuple(mask.shape)[-2:] == (320, 320)
    assert torch.isfinite(logits).all() and int(mask.max()) < 19
    assert torch.equal(mask.reshape(320, 320).long().cpu(), logits.argmax(0).cpu())
    # the heads' convolutions at this size run on the multi-class kernel
    h = model.decode_head
    x1 = torch.zeros(1, 160, 160, 32, dtype=torch.bfloat16, device=dev)
    one = torch.ones(32, device=dev)
    assert ops.conv2d_kernel_id(x1, h.head_x1[0].conv.weight, pad=1, in_scale=one, in_shift=one, in_act=ops.ACT_RELU,
                                out_scale=torch.ones(19, device=dev), out_shift=torch.ones(19, device=dev),
                                act=ops.ACT_RELU, out_dtype=torch.float32) == 7


@pytest.mark.gpu
def test_train_cli_runs_with_19_classes(tmp_path):
    args = [sys.executable, 'tools/train.py', TWO_CFG, '--cfg-options', 'model.decode_head.num_classes=19', '--max-iters', '3',
            '--batch-size', '2', '--height', '320', '--width', '320', '--work-dir', str(tmp_path / 'c19')]
    r = subprocess.run(args, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f'{args}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    m = re.search(r'\[\s*3/3\].*loss_context: ([0-9.eE+-]+).*loss_spatial: ([0-9.eE+-]+)', r.stdout)
    assert m, r.stdout[-2000:]
    print('loss_context / loss_spatial after 3 iterations:', m.group(1), m.group(2))
    assert math.isfinite(float(m.group(1))) and math.isfinite(float(m.group(2)))


@pytest.mark.parametrize('be_name', ['emu', pytest.param('hip', marks=pytest.mark.gpu)])
def test_generic_ohem_loss_is_ordered_in_deterministic_mode(be_name):
    """the unfolded OhemCrossEntropy path that more than two classes take (ledn_ohem_ce_fwd on full-resolution logits):
    in deterministic mode the loss sum over the workgroups is formed in a fixed order (one row per workgroup, no float
    atomics) -- several calls agree bit for bit, and with the default mode's sum to f32 accumulation order.  (On the
    emulator atomics have one order anyway: that variant only checks that the row path computes the same loss.)"""
    import contextlib
    import conftest
    import led_net_amd as L
    from led_net_amd import ops_train as T
    dev = torch.device('cpu' if be_name == 'emu' else 'cuda:0')
    P = (2, 80, 96) if be_name == 'emu' else (2, 640, 640)          # (the GPU case fills the reduce kernel's 2048 workgroups)
    g = torch.Generator().manual_seed(3)
    logits = (2.0 * torch.randn(*P, 19, generator=g)).to(dev)
    tgt = torch.randint(0, 19, P, dtype=torch.int64, generator=g)
    tgt[:, :3] = 255
    tgt = tgt.to(dev)
    with (conftest.bind_emu() if be_name == 'emu' else contextlib.nullcontext()):
        plain = T.ohem_ce_fwd(logits, tgt, 0.9, 1000, 1.0)[0].clone()
        L.set_deterministic(True)
        try:
            outs = [T.ohem_ce_fwd(logits, tgt, 0.9, 1000, 1.0)[0].clone() for _ in range(4)]
        finally:
            L.set_deterministic(False)
    assert all(torch.equal(outs[0], o) for o in outs[1:]), [o.tolist() for o in outs]
    assert torch.isfinite(outs[0]).all() and float(outs[0][3]) >= 1000
    torch.testing.assert_close(outs[0].cpu(), plain.cpu(), rtol=1e-5, atol=1e-6)
