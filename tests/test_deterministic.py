"""Deterministic mode (LEDN_DETERMINISTIC=1 / led_net_amd.set_deterministic, include/ledn.h LEDN_OPT_DETERMINISTIC):
every cross-workgroup reduction in a fixed order.  The reference stack's switch for the same promise is
randomness=dict(seed=304, deterministic=...) (configs/LED_Net/ddrnet_23_in1k-pre_2xb6-120k_cityscapes-1024x1024.py:100).
CPU: the emulator's census of float atomicAdd call sites shows which kernels a step reaches -- none in this mode.
GPU: two runs of the same bf16 steps are BIT-identical, eager == hipGraph replay, and a run resumed from a checkpoint
continues bit-identically."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _setup(dev, dtype, hw=(320, 320), nb=2, seed=5):
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = L.load_config(os.path.join(ROOT, 'tests', 'data', 'lednet_test_config.py'))
    for c in cfg['model']['decode_head']['loss_decode']:
        c['min_kept'] = 20000
    model = L.MODELS.build(cfg['model'])
    if dtype == torch.bfloat16:
        model.set_act_dtype(torch.bfloat16)
    model.to(dev)
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (nb, 3, *hw), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 2, (nb, 1, *hw), dtype=torch.int64, generator=g)
    lab[:, :, :5, :] = 255
    samples = [L.SegDataSample(gt=lab[i].to(dev)) for i in range(nb)]
    return L, model, cfg, img, samples


def test_deterministic_mode_reaches_no_float_atomic(monkeypatch, tmp_path):
    """one bf16 image at 320 x 320 (reflect-padded attention windows, every small-map reduction of the context branch):
    the emulator counts float atomicAdd call sites; the default mode goes through dozens, deterministic mode through none"""
    import atomic_census
    import led_net_amd as L
    L.set_deterministic(True)
    try:
        n, txt = atomic_census.census('bf16', (320, 320), 1, steps=2, out=str(tmp_path / 'census.txt'))
    finally:
        L.set_deterministic(False)
    assert n == 0, f'deterministic mode still reaches float atomics:\n{txt}'


def _run_steps(dev, dtype, steps, deterministic, graph=False, hw=(320, 320), nb=2, collectives=None):
    L, model, cfg, img, samples = _setup(dev, dtype, hw, nb)
    L.set_deterministic(deterministic)
    try:
        tr = L.Trainer(model, cfg, max_iters=1000, collectives=collectives)
        losses = []
        if graph:
            tr.capture(img, samples, warmup=2, restore=True)
            for _ in range(steps):
                out = tr.replay(img, samples)
                losses.append({k: v.detach().clone() for k, v in out.items()})
        else:
            # the eager twin of capture(restore=True): two warm-up steps (the second attaches the gradient sinks), rolled
            # back, so that every compared step is a steady-state step from the initial weights in both modes
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
                losses.append(tr.train_step(img, samples))
        torch.cuda.synchronize()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        return losses, sd, tr.flat_mom.clone()
    finally:
        L.set_deterministic(False)


def _assert_bit_equal(a, b, what):
    la, sa, ma = a
    lb, sb, mb = b
    for i, (x, y) in enumerate(zip(la, lb)):
        for k in x:
            assert torch.equal(x[k], y[k]), f'{what}: step {i} {k}: {x[k].item()!r} vs {y[k].item()!r}'
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, f'{what}: {len(bad)} of {len(sa)} tensors differ, e.g. {bad[:5]}'
    assert torch.equal(ma, mb), f'{what}: momentum buffers differ'


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_two_runs_are_bit_identical(dtype):
    dev = torch.device('cuda:0')
    a = _run_steps(dev, dtype, 3, True)
    b = _run_steps(dev, dtype, 3, True)
    _assert_bit_equal(a, b, 'two deterministic eager runs')


@pytest.mark.gpu
def test_graph_replay_equals_eager_bit_exact():
    dev = torch.device('cuda:0')
    a = _run_steps(dev, torch.bfloat16, 3, True, graph=False)
    b = _run_steps(dev, torch.bfloat16, 3, True, graph=True)
    _assert_bit_equal(a, b, 'hipGraph replay vs eager')


@pytest.mark.gpu
def test_default_mode_is_not_bit_reproducible():
    """the contrast: without the switch two runs of the same three bf16 steps differ (f32 atomics order of the small-map
    reductions) -- documents what the mode buys; if this ever becomes bit-equal the default got deterministic for free"""
    dev = torch.device('cuda:0')
    a = _run_steps(dev, torch.bfloat16, 3, False)
    b = _run_steps(dev, torch.bfloat16, 3, False)
    la, lb = a[0][-1], b[0][-1]
    import math
    for k in la:        # (measured: the third step's losses of two default-mode runs differ by up to 8 % on this random-label batch)
        assert math.isfinite(float(la[k])) and abs(float(la[k]) - float(lb[k])) <= 0.5 * abs(float(lb[k])) + 1e-3, (k, float(la[k]), float(lb[k]))
    same = all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    print('default mode: two runs bit-identical:', same, '; third-step losses', {k: (float(la[k]), float(lb[k])) for k in la})


@pytest.mark.gpu
def test_resumed_run_continues_bit_identically(tmp_path):
    """steps 1-2, checkpoint, steps 3-4 in the same process vs a FRESH model + Trainer resumed from the file running
    steps 3-4: weights, momentum and losses bit-equal (round 3 could only compare against a run-to-run spread)"""
    import led_net_amd as L
    dev = torch.device('cuda:0')
    L.set_deterministic(True)
    try:
        _, model, cfg, img, samples = _setup(dev, torch.bfloat16)
        tr = L.Trainer(model, cfg, max_iters=1000)
        for _ in range(2):
            tr.train_step(img, samples)
        path = str(tmp_path / 'iter_2.pth')
        L.save_checkpoint(model, path, trainer=tr, meta=dict(iter=2))
        want = [tr.train_step(img, samples) for _ in range(2)]
        torch.cuda.synchronize()
        want_sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        _, model2, cfg2, img2, samples2 = _setup(dev, torch.bfloat16)
        tr2 = L.Trainer(model2, cfg2, max_iters=1000)
        ck = L.load_checkpoint(model2, path, map_location='cpu', strict=True)
        L.resume(tr2, ck)
        assert tr2.iter == 2
        # as tools/train.py --resume does: capture free of side effects (warm-up steps rolled back), then replay
        tr2.capture(img2, samples2, warmup=2, restore=True)
        got = [{k: v.detach().clone() for k, v in tr2.replay(img2, samples2).items()} for _ in range(2)]
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(want, got)):
            for k in x:
                assert torch.equal(x[k], y[k]), (i, k, float(x[k]), float(y[k]))
        bad = [k for k, v in model2.state_dict().items() if not torch.equal(v, want_sd[k])]
        assert not bad, bad[:5]
    finally:
        L.set_deterministic(False)


@pytest.mark.gpu
@pytest.mark.parametrize('multi,forks', [('0', 7), ('1', 7), ('1', 0)])
def test_rccl_step_graph_replay_equals_eager_bit_exact(multi, forks, monkeypatch):
    """the N > 1 step on ONE rank (one-rank RCCL communicators: everything but the wire) in deterministic mode: the step
    captured with its ncclAllReduce launches and replayed three times == the same three steps launched eagerly, bit for
    bit -- for the default single-launch-stream plan (LEDN_MULTI_COMM=0), for the multi-communicator plan with the
    context-branch streams (LEDN_CTX_FORKS=7) and without them (0).  A collective recorded on the wrong stream, dropped
    from the graph or replayed against a stale buffer changes the weights."""
    from led_net_amd import train as TR
    monkeypatch.setenv('LEDN_EXPERIMENTAL', '1')
    monkeypatch.setenv('LEDN_MULTI_COMM', multi)
    monkeypatch.setattr(TR, 'CTX_FORKS', forks)
    dev = torch.device('cuda:0')
    a = _run_steps(dev, torch.bfloat16, 3, True, graph=False, nb=4, collectives='rccl')
    b = _run_steps(dev, torch.bfloat16, 3, True, graph=True, nb=4, collectives='rccl')
    _assert_bit_equal(a, b, f'rccl step (LEDN_MULTI_COMM={multi}, CTX_FORKS={forks}): hipGraph replay vs eager')


# --------------------------------------------------------------------------- #
# the deterministic-mode kernels compute the SAME thing: the reference-generated block goldens (outputs, input gradients,
# parameter gradients, running statistics) hold with the mode switched on -- emulator and MI355X.  Covers the kernels
# that exist only in this mode: mfaf_dctx_det_kernel + mfaf_ctx_finish_kernel (Muti_AFF), window_attn_fold_kernel and the
# fixed-point relative-position-bias adjoint (GETB on the odd 13 x 27 map), partial-row statistics of small grids.
# --------------------------------------------------------------------------- #
def _golden_cases():
    import test_train as TT
    cases = [('mfaf', n) for n in TT.train_names('g6_')] + [('getb', n) for n in TT.train_names('g5_')]
    cases += [('sesp', TT.train_names('g2_')[0]), ('sesp', TT.train_names('g4')[0]), ('basic', TT.train_names('g11_')[-1]),
              ('ppm', TT.train_names('g14_')[0]), ('head', 'g10')]
    return cases


@pytest.mark.parametrize('kind,name', _golden_cases())
def test_block_goldens_hold_in_deterministic_mode(be, kind, name):
    import led_net_amd as L
    import test_train as TT
    TT._DEV[0] = be.dev
    L.set_deterministic(True)
    try:
        if kind == 'head':
            TT.test_led_head_train_golden(be)
        else:
            {'mfaf': TT.test_mfaf_train_golden, 'getb': TT.test_getb_train_golden, 'sesp': TT.test_sesp_train_golden,
             'basic': TT.test_basic_block_train_golden, 'ppm': TT.test_ppm_train_golden}[kind](be, name)
    finally:
        L.set_deterministic(False)
        TT._DEV[0] = torch.device('cpu')
