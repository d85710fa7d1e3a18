"""The step guard: optimizer steps whose gradient holds an Inf or a NaN are skipped, decided on the device (what mmengine's
AmpOptimWrapper / torch.cuda.amp.GradScaler.step do).  The finite pass, the one-workgroup verdict, the guarded optimizer
launch, the Trainer around them (eager, captured, two ranks, checkpoint), the config path and the C ABI's argument checks.

Expected values: torch.isfinite for the finite pass; ledn_optim_step / ledn_optim_step_ema themselves for an applied step
(bit for bit); torch.optim.AdamW fed only the applied gradients for the step count.  The one tolerance in this file is
test_optim_step.test_adamw_trajectory_error_vs_float64's: the kernel's distance from a float64 torch run may be at most
4x the distance of torch's own f32 run.  Everything else is compared as int32 bit patterns.
Emulator on the CPU; the same bodies on the MI355X with -m gpu."""
import copy
import ctypes as C
import math
import os
import struct
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_test_config.py')
AMP_CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_amp_config.py')
CE_DICE_CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_ce_dice_config.py')
HYP = dict(momentum=0.9, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
NAN, INF = float('nan'), float('inf')


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    if not a.is_floating_point():
        return torch.equal(a.detach().cpu(), b.detach().cpu())
    return torch.equal(_bits(a), _bits(b))


def _off(n, off, dev, fill=None):
    """n floats starting `off` floats behind a 16-byte aligned address"""
    base = torch.zeros(n + 4, device=dev)
    assert base.data_ptr() % 16 == 0
    t = base[off:off + n]
    if fill is not None:
        t.copy_(fill.to(dev))
    return t


def _kind_id(kind):
    from led_net_amd import _lib
    return _lib.OPTIM_ADAMW if kind == 'AdamW' else _lib.OPTIM_SGD


# --------------------------------------------------------------------------- #
# 1. the finite pass
# --------------------------------------------------------------------------- #
BIG = 3 * 4096 + 5                    # four workgroups along the tensor in the finite pass, seven in the optimizer launch
# (elements, offset in floats from a 16-byte aligned address) per tensor: 1 to 5 tensors, every size of the list, aligned
# gradients (16-byte loads) next to gradients one and three floats off (scalar head and tail)
TABLES = [[(1, 0)],
          [(3, 1), (5, 0)],
          [(4096, 0), (4097, 1), (1, 3)],
          [(BIG, 3), (5, 1), (4097, 0), (3, 0)],
          [(1, 1), (3, 0), (5, 3), (4096, 1), (BIG, 0)]]


def _finite_table(spec, dev):
    from led_net_amd import ops_train as T
    gs = [_off(n, off, dev) for n, off in spec]
    assert [g.data_ptr() % 16 for g in gs] == [4 * off for _, off in spec]
    ps = [torch.zeros(n, device=dev) for n, _ in spec]
    ms = [torch.zeros(n, device=dev) for n, _ in spec]
    tab = T.OptimTable(ps, gs, ms)
    return tab, gs, T.StepGuard(dev, len(spec))


def _positions(n, off):
    """element 0, the last element, both sides of the first and of the last 16-byte boundary, the scalar tail"""
    head = min(n, (4 - off) % 4)
    nvec = (n - head) // 4
    cand = {0, n - 1, head - 1, head, head + 4 * nvec - 1, head + 4 * nvec, head + 4, head + 3}
    return sorted(i for i in cand if 0 <= i < n)


def _run_finite(tab, guard):
    guard.bad.fill_(-7)                           # (every word must be written)
    guard.flags.fill_(-7)
    guard.finite_pass(tab)
    chunks = min(8, -(-tab.max_n // 4096))
    flags = guard.flags[:tab.n * chunks].cpu()
    assert bool(((flags == 0) | (flags == 1)).all())
    return guard.bad.cpu().tolist(), flags.view(tab.n, chunks)


@pytest.mark.parametrize('spec', TABLES, ids=[str(len(s)) for s in TABLES])
def test_finite_pass_flags_exactly_the_poisoned_tensor(be, spec):
    tab, gs, guard = _finite_table(spec, be.dev)
    gen = torch.Generator().manual_seed(len(spec))
    clean = [torch.randn(n, generator=gen) for n, _ in spec]
    vals = (NAN, INF, -INF)
    k = 0
    for i, (n, off) in enumerate(spec):
        for pos in _positions(n, off):
            for g, c in zip(gs, clean):
                g.copy_(c.to(be.dev))
            gs[i][pos] = vals[k % 3]
            k += 1
            bad, flags = _run_finite(tab, guard)
            want = [int(not bool(torch.isfinite(g).all())) for g in gs]
            assert want == [int(j == i) for j in range(len(spec))]
            assert bad == want, (i, pos, vals[(k - 1) % 3])
            assert flags.sum(1).clamp(max=1).tolist() == want       # the per-workgroup flags give the same verdict
    # every value at one place of every tensor at once
    for v in vals:
        for g, c in zip(gs, clean):
            g.copy_(c.to(be.dev))
            g[g.numel() // 2] = v
        assert _run_finite(tab, guard)[0] == [1] * len(spec)


@pytest.mark.parametrize('spec', [TABLES[2], TABLES[4]], ids=['3', '5'])
def test_finite_pass_negative_controls(be, spec):
    tab, gs, guard = _finite_table(spec, be.dev)
    fmax = torch.finfo(torch.float32).max
    for fill in (0.0, fmax, -fmax, 1e-45, -0.0):
        for g in gs:
            g.fill_(fill)
        if fill == 1e-45:
            assert float(gs[0][0]) > 0.0                       # (a denormal, not flushed on the way in)
        bad, flags = _run_finite(tab, guard)
        assert bad == [0] * len(spec) and int(flags.sum()) == 0, fill
    # a squared sum that overflows is not a non-finite gradient
    for g in gs:
        g.fill_(1e30)
    assert _run_finite(tab, guard)[0] == [0] * len(spec)


# --------------------------------------------------------------------------- #
# 2. / 3. the guarded step against ledn_optim_step / ledn_optim_step_ema
# --------------------------------------------------------------------------- #
SIZES = (4100, 1, 3, 4097, BIG, 8)
P_OFF = (0, 0, 0, 0, 0, 1)             # tensor 5: an aligned gradient next to a parameter one float off alignment
LR_MULTS = (1.0, 0.0, 10.0, 0.5, 1.0, 2.0)
WD_MULTS = (1.0, 1.0, 0.0, 0.0, 1.0, 0.5)


def _host_table(kind, seed, warm):
    g = torch.Generator().manual_seed(seed)
    hp = [torch.randn(n, generator=g) for n in SIZES]
    hg = [torch.randn(n, generator=g) * (0.1 + i) for i, n in enumerate(SIZES)]
    hm = [torch.randn(n, generator=g) * 0.1 if warm else torch.zeros(n) for n in SIZES]
    hv = [torch.rand(n, generator=g) * 0.01 if warm else torch.zeros(n) for n in SIZES]
    ha = [torch.randn(n, generator=g) for n in SIZES]
    return hp, hg, hm, hv, ha


def _device_table(kind, host, dev, ema):
    """gradients back to back in ONE flat buffer (tensors 2 and 5 then start off 16-byte alignment)"""
    from led_net_amd import ops_train as T
    hp, hg, hm, hv, ha = host
    flat = torch.zeros(sum(SIZES) + 4, device=dev)[:sum(SIZES)]
    gd, o = [], 0
    for n, x in zip(SIZES, hg):
        gd.append(flat[o:o + n])
        gd[-1].copy_(x.to(dev))
        o += n
    pd = [_off(n, po, dev, x) for n, po, x in zip(SIZES, P_OFF, hp)]
    md = [_off(n, 0, dev, x) for n, x in zip(SIZES, hm)]
    vd = [_off(n, 0, dev, x) for n, x in zip(SIZES, hv)] if kind == 'AdamW' else None
    ad = [_off(n, 0, dev, x) for n, x in zip(SIZES, ha)] if ema else None
    tab = T.OptimTable(pd, gd, md, vd, LR_MULTS, WD_MULTS, avgs=ad)
    return tab, flat, pd, gd, md, vd, ad


def _clip_obj(mode, flat, hg, dev):
    from led_net_amd import _lib, ops_train as T
    if mode == 'off':
        return None
    if mode == 'value':
        return T.GradClip(dev, flat.numel(), norm_type=_lib.NORM_NONE, clip_value=0.7)
    p_ = 2.0 if mode == 'l2' else math.inf
    total = float(torch.linalg.vector_norm(torch.cat(hg).double() * 0.5, p_))
    return T.GradClip(dev, flat.numel(), norm_type=_lib.NORM_L2 if mode == 'l2' else _lib.NORM_INF, max_norm=0.5 * total)


def _one_step(kind, clip_mode, ema, dev, guarded, poison=None, w=0.25, t=1):
    """one launch on the same inputs -> everything it may touch; guarded: through the three guard launches"""
    from led_net_amd import ops_train as T
    host = _host_table(kind, seed=5, warm=False)
    tab, flat, pd, gd, md, vd, ad = _device_table(kind, host, dev, ema)
    if poison is not None:
        gd[poison[0]][poison[1]] = poison[2]
    clip = _clip_obj(clip_mode, flat, host[1], dev)
    if clip is not None:
        clip.norm_pass(flat)
    guard = None
    if guarded:
        guard = T.StepGuard(dev, tab.n)
        guard.finite_pass(tab)
        guard.verdict(tab, HYP['betas'], it=41)
    tab.step(_kind_id(kind), 3e-3, 1e-4, grad_scale=0.5, t=t, clip=clip, ema_w=w if ema else None, guard=guard, **HYP)
    out = dict(p=pd, m=md, v=vd or [], g=gd, avg=ad or [], norm=[clip.norm_out] if clip_mode in ('l2', 'inf') else [])
    return {k: [x.detach().cpu().clone() for x in v] for k, v in out.items()}, guard, host


@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'ema'])
@pytest.mark.parametrize('clip_mode', ['off', 'l2', 'inf', 'value'])
@pytest.mark.parametrize('kind', ['SGD', 'AdamW'])
def test_guarded_step_with_clean_gradients_has_the_bits_of_optim_step(be, kind, clip_mode, ema):
    want, _, _ = _one_step(kind, clip_mode, ema, be.dev, guarded=False)
    got, guard, _ = _one_step(kind, clip_mode, ema, be.dev, guarded=True)
    for key in want:
        assert len(got[key]) == len(want[key])
        for i, (a, b) in enumerate(zip(got[key], want[key])):
            assert _same(a, b), (key, i)
    assert all(float(g.abs().max()) == 0.0 for g in got['g'])
    assert guard.state() == dict(applied=1, skipped=0)
    assert float(guard.grad_finite) == 1.0 and float(guard.skipped_steps) == 0.0 and int(guard.skip) == 0
    assert guard.report() is None


@pytest.mark.parametrize('ema,w', [(False, 0.25), (True, 0.25), (True, 1.0)], ids=['plain', 'ema', 'ema-copy'])
@pytest.mark.parametrize('clip_mode', ['off', 'l2', 'value'])
@pytest.mark.parametrize('kind', ['SGD', 'AdamW'])
def test_guarded_step_with_one_nan_leaves_the_step_out(be, kind, clip_mode, ema, w):
    poison = (3, 4096, NAN)            # tensor 3's one-float tail
    got, guard, host = _one_step(kind, clip_mode, ema, be.dev, guarded=True, poison=poison, w=w)
    hp, hg, hm, hv, ha = host
    for i in range(len(SIZES)):
        assert _same(got['p'][i], hp[i]) and _same(got['m'][i], hm[i]), i       # no update, no weight decay
        if kind == 'AdamW':
            assert _same(got['v'][i], hv[i]), i
        assert float(got['g'][i].abs().max()) == 0.0 and not bool(torch.isnan(got['g'][i]).any())
        if ema:
            wt = torch.tensor(w, dtype=torch.float32)
            want = hp[i].clone() if w >= 1.0 else ha[i] + wt * (hp[i] - ha[i])
            assert _same(got['avg'][i], want), i
    if clip_mode == 'l2':
        assert math.isnan(float(got['norm'][0][0]))            # norm_out is written as in an applied step
    assert guard.state() == dict(applied=0, skipped=1)
    assert float(guard.grad_finite) == 0.0 and float(guard.skipped_steps) == 1.0 and int(guard.skip) == 1
    assert guard.report() == (41, [3])


def test_sticky_record_survives_applied_steps_and_follows_the_last_skip(be):
    from led_net_amd import ops_train as T
    host = _host_table('SGD', seed=6, warm=False)
    tab, flat, pd, gd, md, vd, ad = _device_table('SGD', host, be.dev, False)
    guard = T.StepGuard(be.dev, tab.n)
    stamp = torch.zeros(1, dtype=torch.int64, device=be.dev)
    seen = []
    for it, poison in enumerate([None, [(0, 0, INF), (5, 7, NAN)], None, [(2, 1, -INF)], None]):
        for g, x in zip(gd, host[1]):
            g.copy_(x.to(be.dev))
        for i, pos, v in poison or []:
            gd[i][pos] = v
        stamp.fill_(100 + it)
        guard.finite_pass(tab)
        guard.verdict(tab, HYP['betas'], it=-1, iter_dev=stamp)                # the device stamp wins
        tab.step(_kind_id('SGD'), 1e-3, guard=guard, **HYP)
        seen.append((guard.state(), guard.report(), float(guard.grad_finite), float(guard.skipped_steps)))
    assert [s[1] for s in seen] == [None, (101, [0, 5]), (101, [0, 5]), (103, [2]), (103, [2])]
    assert [s[0]['applied'] for s in seen] == [1, 1, 2, 2, 3] and [s[0]['skipped'] for s in seen] == [0, 1, 1, 2, 2]
    assert [s[2] for s in seen] == [1.0, 0.0, 1.0, 0.0, 1.0] and [s[3] for s in seen] == [0.0, 1.0, 1.0, 2.0, 2.0]


# --------------------------------------------------------------------------- #
# 4. AdamW's step count follows the applied steps
# --------------------------------------------------------------------------- #
def test_adamw_clean_bad_clean_equals_two_plain_steps_and_torch(be):
    from led_net_amd import ops_train as T
    host = _host_table('AdamW', seed=8, warm=False)
    hp = host[0]
    gen = torch.Generator().manual_seed(80)
    grads = [[torch.randn(n, generator=gen) for n in SIZES] for _ in range(3)]
    grads[1][4][BIG - 1] = INF
    lr = 1e-3

    def run(guarded):
        tab, flat, pd, gd, md, vd, _ = _device_table('AdamW', host, be.dev, False)
        guard = T.StepGuard(be.dev, tab.n) if guarded else None
        t = 0
        for k in range(3):
            if not guarded and k == 1:
                continue
            for g, x in zip(gd, grads[k]):
                g.copy_(x.to(be.dev))
            if guarded:
                guard.finite_pass(tab)
                guard.verdict(tab, HYP['betas'], it=k)
            t += 1
            tab.step(_kind_id('AdamW'), lr, t=1 if guarded else t, guard=guard, **HYP)      # (guarded: t is not used)
        return [x.cpu() for x in pd + md + vd], guard
    got, guard = run(True)
    want, _ = run(False)
    for i, (a, b) in enumerate(zip(got, want)):
        assert _same(a, b), i
    assert guard.state() == dict(applied=2, skipped=1) and guard.report() == (1, [4])
    # the bias corrections the device formed for the second applied step
    bc = guard.bias_corrections.cpu().tolist()
    want_bc = [struct.unpack('f', struct.pack('f', x))[0] for x in T.optim_scalars(lr, 0.0, HYP['betas'], 2)[2:]]
    assert bc == want_bc
    # torch.optim.AdamW fed only the two clean gradients (LR_MULTS / WD_MULTS as param groups), f32 and f64
    runs = {}
    for dtype in (torch.float32, torch.float64):
        ref = [p.clone().to(dtype).requires_grad_(True) for p in hp]
        opt = torch.optim.AdamW([dict(params=[r_], lr=lm * lr, weight_decay=wm * HYP['weight_decay'])
                                 for r_, lm, wm in zip(ref, LR_MULTS, WD_MULTS)], betas=HYP['betas'], eps=HYP['eps'])
        for k in (0, 2):
            for r_, x in zip(ref, grads[k]):
                r_.grad = x.to(dtype)
            opt.step()
        runs[dtype] = [r_.detach().double() for r_ in ref]
    err_kernel = max(float((p.double() - w).abs().max()) for p, w in zip(got[:len(SIZES)], runs[torch.float64]))
    err_torch = max(float((a - w).abs().max()) for a, w in zip(runs[torch.float32], runs[torch.float64]))
    print(f'AdamW clean/bad/clean: max |p - p_f64|: kernel {err_kernel:.3e}, torch f32 {err_torch:.3e}')
    assert err_torch > 0 and err_kernel <= 4.0 * err_torch


# --------------------------------------------------------------------------- #
# 5. the Trainer, eager
# --------------------------------------------------------------------------- #
LIGHT = dict(context_tail='pappm', getb_stage3=False)     # backbone flags of the emulator's network (below)
LIGHT_HW = 64


def _light_cfg(optim_wrapper=None):
    """tests/data/lednet_test_config.py with the pooling-pyramid context tail and no window attention: the smallest
    network the Trainer runs, for 64 x 64 images (window attention needs 320 x 320, 35 s per step on the emulator
    against 5).  Every parameter still goes through the same flat buffers, table and optimizer launch."""
    import led_net_amd as L
    cfg = L.load_config(CFG)
    cfg['model']['backbone'].update(LIGHT)
    for c in cfg['model']['decode_head']['loss_decode']:
        c['min_kept'] = 1000
    if optim_wrapper is not None:
        cfg['optim_wrapper'] = optim_wrapper
        cfg.pop('optimizer', None)
    return cfg


def _light_batch(batch=1, seed=11):
    import led_net_amd as L
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (batch, 3, LIGHT_HW, LIGHT_HW), dtype=torch.uint8, generator=g)
    lab = torch.randint(0, 2, (batch, 1, LIGHT_HW, LIGHT_HW), dtype=torch.int64, generator=g)
    lab[:, :, :3, :] = 255
    return img, lab


def _small(dev, **kw):
    """the GPU runs tests/test_clip_grad.py's _small_trainer; the emulator the light network above, built the same way"""
    import led_net_amd as L
    if dev.type == 'cuda':
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from test_clip_grad import _small_trainer
        return _small_trainer(dev, batch=1, **kw)
    torch.manual_seed(304)
    cfg = _light_cfg()
    model = L.MODELS.build(cfg['model'])
    img, lab = _light_batch()
    return L.Trainer(model, cfg, max_iters=1000, **kw), model, cfg, img, [L.SegDataSample(gt=lab[0])]


def _state(tr, model):
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    sd['__mom'] = tr.flat_mom.detach().cpu().clone()
    if tr.flat_ema is not None:
        sd['__ema'] = tr.flat_ema.detach().cpu().clone()
    return sd


def _owner(tr, k):
    off = 0
    for name, p in zip(tr.names, tr.params):
        if off <= k < off + p.numel():
            return name
        off += p.numel()
    raise AssertionError(k)


def _trainer_eager_case(dev):
    import led_net_amd as L
    ema = dict(ema_type='ExponentialMovingAverage', momentum=0.25, gamma=None, update_buffers=False, begin_iter=0)
    ref_tr, ref_model, _, img, samples = _small(dev, ema=ema)
    tr, model, _, _, _ = _small(dev, ema=ema, skip_nonfinite=True)
    assert ref_tr.guard is None and ref_tr.skip_nonfinite is False and tr.skip_nonfinite is True
    model.load_state_dict(ref_model.state_dict())
    tr.load_ema_state(0, {})
    ref_tr.load_ema_state(0, {})
    for it in range(3):
        want = ref_tr.train_step(img, samples)
        got = tr.train_step(img, samples)
        assert sorted(got) == sorted(list(want) + ['grad_finite', 'skipped_steps'])
        assert 'grad_finite' not in want and 'skipped_steps' not in want          # the default keeps today's keys
        assert float(got['grad_finite']) == 1.0 and float(got['skipped_steps']) == 0.0
        for k in want:
            assert _same(got[k], want[k]), (it, k)
    a, b = _state(tr, model), _state(ref_tr, ref_model)
    assert not [k for k in a if not _same(a[k], b[k])]
    assert tr.nonfinite_report() is None
    # a step whose gradient gets a NaN between the two halves
    before = _state(tr, model)
    tr.forward_backward(img, samples)
    stats = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if 'running_' in k or 'num_batches' in k}
    k = tr.flat_grad.numel() - 5
    assert float(tr.flat_grad[k]) == float(tr.flat_grad[k])                        # finite before
    tr.flat_grad[k] = NAN
    it0, steps0 = tr.iter, tr.ema_steps
    w = torch.tensor(tr._ema_w(), dtype=torch.float32)
    out = tr.optimizer_step()
    assert tr.iter == it0 + 1 and tr.ema_steps == steps0 + 1
    assert float(out['grad_finite']) == 0.0 and float(out['skipped_steps']) == 1.0
    after = _state(tr, model)
    for key in after:
        if key in stats:
            assert _same(after[key], stats[key]), key                              # (the forward's, not the guard's)
        elif key == '__ema':
            n = tr.flat_mom.numel()
            live = torch.zeros(n, dtype=torch.bool)
            off = 0
            for p in tr.params:
                if any(p is q for q in tr.live):
                    live[off:off + p.numel()] = True
                off += p.numel()
            flat_p = torch.cat([p.detach().cpu().reshape(-1) for p in tr.params])
            want = before[key][:n] + w * (flat_p - before[key][:n])
            assert _same(after[key][:n][live], want[live])
        else:
            assert _same(after[key], before[key]), key
    assert float(tr.flat_grad.abs().max()) == 0.0 and not bool(torch.isnan(tr.flat_grad).any())
    rep = tr.nonfinite_report()
    assert rep == dict(iter=it0, params=[_owner(tr, k)]), rep
    # the next clean step applies
    out = tr.train_step(img, samples)
    assert float(out['grad_finite']) == 1.0 and float(out['skipped_steps']) == 1.0
    moved = _state(tr, model)
    assert not _same(moved['__mom'], after['__mom'])
    assert tr.guard.state() == dict(applied=4, skipped=1) and tr.iter == 5
    assert tr.nonfinite_report() == rep                                            # sticky


def test_trainer_eager(emu):
    _trainer_eager_case(torch.device('cpu'))


@pytest.mark.gpu
def test_trainer_eager_gpu():
    import led_net_amd as L
    L.set_deterministic(True)           # the two trainers' gradients are then the same bits
    try:
        _trainer_eager_case(torch.device('cuda:0'))
    finally:
        L.set_deterministic(False)


# --------------------------------------------------------------------------- #
# 6. the captured graph
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
def test_captured_steps_with_a_nan_batch_equal_eager():
    import led_net_amd as L
    dev = torch.device('cuda:0')
    L.set_deterministic(True)
    try:
        cfg = L.load_config(CE_DICE_CFG)
        cfg['optim_wrapper'] = dict(type='AmpOptimWrapper', optimizer=cfg['optimizer'], loss_scale='dynamic')
        gen = torch.Generator().manual_seed(31)
        batches = []
        for i in range(4):
            img = torch.rand(2, 3, 320, 320, generator=gen) * 255.0
            lab = torch.randint(0, 2, (2, 1, 320, 320), dtype=torch.int64, generator=gen)
            lab[:, :, :6, :] = 255
            if i == 1:
                img[0, 1, 100, 200] = NAN
            batches.append((img.to(dev), [L.SegDataSample(gt=lab[j].to(dev)) for j in range(2)]))
        torch.manual_seed(304)
        init = copy.deepcopy(L.MODELS.build(cfg['model']).state_dict())

        def run(graph):
            model = L.MODELS.build(cfg['model']).to(dev)
            model.load_state_dict(init)
            tr = L.Trainer(model, cfg, max_iters=1000)
            assert tr.skip_nonfinite
            snaps, skipped = [], []
            if graph:
                tr.capture(*batches[0], warmup=2, restore=True)
            else:                       # the same warm-up, put back the same way
                keep = ([p.detach().clone() for p in tr.params], [b.detach().clone() for b in model.buffers()], tr.iter)
                for _ in range(2):
                    tr.train_step(*batches[0])
                with torch.no_grad():
                    for p, v in zip(tr.params, keep[0]):
                        p.copy_(v)
                    for b, v in zip(model.buffers(), keep[1]):
                        b.copy_(v)
                    tr.flat_mom.zero_()
                tr.iter = keep[2]
                tr.guard.load_state(tr.iter, 0)
            for b in batches:
                out = tr.replay(*b) if graph else tr.train_step(*b)
                torch.cuda.synchronize()
                skipped.append(float(out['skipped_steps']))
                snaps.append([p.detach().clone() for p in tr.params] + [tr.flat_mom.clone()])
            return snaps, skipped, tr.nonfinite_report(), tr.guard.state()
        eager, graph = run(False), run(True)
        print('skipped_steps eager', eager[1], 'captured', graph[1], 'report', graph[2])
        assert eager[1] == graph[1] == [0.0, 1.0, 1.0, 1.0]
        for i, (a, b) in enumerate(zip(eager[0], graph[0])):
            assert all(torch.equal(x, y) for x, y in zip(a, b)), i
        assert all(torch.equal(x, y) for x, y in zip(graph[0][0], graph[0][1]))      # the NaN step changed nothing
        assert not all(torch.equal(x, y) for x, y in zip(graph[0][1], graph[0][2]))  # the next one applied
        assert not any(bool(torch.isnan(x).any()) for x in graph[0][3])
        assert eager[3] == graph[3] == dict(applied=3, skipped=1)
        # which gradients the NaN reaches is the network's business (this ReLU maps NaN to 0, so it may stop at the stem);
        # the record names the same parameters either way, with the iteration of the skipped replay
        assert graph[2] == eager[2] and graph[2]['iter'] == 1 and len(graph[2]['params']) >= 1
    finally:
        L.set_deterministic(False)


# --------------------------------------------------------------------------- #
# 7. configuration
# --------------------------------------------------------------------------- #
def _tiny_model():
    import led_net_amd as L
    return L.MODELS.build(L.load_config(CFG)['model']), L.load_config(CFG)


def test_amp_wrapper_turns_the_guard_on_and_the_argument_wins():
    import led_net_amd as L
    model, cfg = _tiny_model()
    assert L.Trainer(model, cfg).skip_nonfinite is False and L.Trainer(model).skip_nonfinite is False
    assert L.Trainer(model, cfg)._general is False                         # the default path is the plain SGD launch
    cfg['optim_wrapper'] = dict(type='OptimWrapper', optimizer=cfg['optimizer'])
    assert L.Trainer(model, cfg).skip_nonfinite is False
    cfg['optim_wrapper']['type'] = 'AmpOptimWrapper'
    tr = L.Trainer(model, cfg)
    assert tr.skip_nonfinite is True and tr._general is True
    assert (tr.base_lr, tr.momentum, tr.wd) == (0.01, 0.9, 5e-4)
    assert L.Trainer(model, cfg, skip_nonfinite=False).skip_nonfinite is False
    assert L.Trainer(model, cfg, skip_nonfinite=False)._general is False
    assert L.Trainer(model, skip_nonfinite=True).skip_nonfinite is True
    for extra in (dict(loss_scale='dynamic'), dict(loss_scale=512.0), dict(loss_scale=1), dict(dtype='bfloat16'),
                  dict(dtype=None), dict(loss_scale=dict(init_scale=65536.0, growth_interval=2000))):
        cfg['optim_wrapper'] = dict(type='AmpOptimWrapper', optimizer=cfg['optimizer'], **extra)
        assert L.Trainer(model, cfg).skip_nonfinite is True
    amp = L.load_config(AMP_CFG)
    assert amp['optim_wrapper']['type'] == 'AmpOptimWrapper' and L.Trainer(model, amp).skip_nonfinite is True
    plain = L.load_config(CFG)
    assert amp['model'] == plain['model'] and amp['optim_wrapper']['optimizer'] == plain['optimizer']


@pytest.mark.parametrize('bad,word', [(dict(dtype='float16'), 'dtype'), (dict(loss_scale=0), 'loss_scale'),
                                      (dict(loss_scale='static'), 'loss_scale'), (dict(loss_scale=-1.0), 'loss_scale'),
                                      (dict(loss_scale=NAN), 'loss_scale'), (dict(loss_scale=True), 'loss_scale'),
                                      (dict(loss_scale=dict(scale=2.0)), 'scale'), (dict(dtype='float32'), 'dtype'),
                                      (dict(clip_grad=dict(max_norm=1.0, error_if_nonfinite=True)), 'error_if_nonfinite')])
def test_bad_amp_wrapper_raises_value_error(bad, word):
    import led_net_amd as L
    model, cfg = _tiny_model()
    cfg['optim_wrapper'] = dict(type='AmpOptimWrapper', optimizer=cfg['optimizer'], **bad)
    with pytest.raises(ValueError, match=word):
        L.Trainer(model, cfg)
    with pytest.raises(ValueError, match=word):
        L.Trainer(model, cfg, skip_nonfinite=False)        # a malformed section is an error whoever switches the guard


def test_error_if_nonfinite_still_raises_with_the_guard_on():
    import led_net_amd as L
    model, _ = _tiny_model()
    with pytest.raises(ValueError, match='not supported'):
        L.Trainer(model, clip_grad=dict(max_norm=1.0, error_if_nonfinite=True), skip_nonfinite=True)


# --------------------------------------------------------------------------- #
# 8. checkpoint round trip
# --------------------------------------------------------------------------- #
ADAMW = dict(type='AdamW', lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)


def _adamw_guarded(dev, init=None):
    import led_net_amd as L
    torch.manual_seed(304)
    cfg = _light_cfg(dict(type='AmpOptimWrapper', optimizer=dict(ADAMW)))
    model = L.MODELS.build(cfg['model']).to(dev)
    if init is not None:
        model.load_state_dict(init)
    return L.Trainer(model, cfg, max_iters=1000), model


def _nan_step(tr, batch, poison):
    """one step through the public halves; poison: write a NaN into the gradient in between"""
    tr.forward_backward(*batch)
    if poison:
        tr.flat_grad[tr.flat_grad.numel() - 3] = NAN
    return tr.optimizer_step()


def test_checkpoint_round_trip_and_resume_after_a_skipped_step(emu, tmp_path):
    import led_net_amd as L
    dev = torch.device('cpu')
    img, lab = _light_batch()
    batch = (img, [L.SegDataSample(gt=lab[0])])
    tr, model = _adamw_guarded(dev)
    assert tr.opt_kind == 'AdamW' and tr.skip_nonfinite
    init = copy.deepcopy(model.state_dict())
    tr.train_step(*batch)                              # applied (and attaches the gradient views)
    _nan_step(tr, batch, True)                         # skipped
    assert tr.guard.state() == dict(applied=1, skipped=1) and tr.iter == 2
    ck = dict(model=copy.deepcopy(model.state_dict()), opt=tr.optimizer_state_dict(), sched=tr.scheduler_state_dicts())
    torch.save(ck, tmp_path / 'ck.pt')
    ck = torch.load(tmp_path / 'ck.pt', weights_only=False)
    assert ck['opt']['step_guard'] == dict(applied=1, skipped=1)
    assert {float(st['step']) for st in ck['opt']['state'].values()} == {1.0}      # torch's count: the applied steps
    _nan_step(tr, batch, False)                        # the uninterrupted run's third step: applied with t = 2
    want = _state(tr, model)
    want['__v'] = tr.flat_v.clone()
    # resumed: counters restored, the same third step
    tr2, model2 = _adamw_guarded(dev, init)
    tr2.train_step(*batch)                             # (builds the table; everything it did is overwritten by the load)
    model2.load_state_dict(ck['model'])
    tr2.load_optimizer_state_dict(ck['opt'], ck['sched'])
    assert tr2.iter == 2 and tr2.guard.state() == dict(applied=1, skipped=1)
    assert float(tr2.guard.skipped_steps) == 1.0
    _nan_step(tr2, batch, False)
    got = _state(tr2, model2)
    got['__v'] = tr2.flat_v.clone()
    assert not [k for k in want if not _same(want[k], got[k])]
    assert tr2.guard.state() == dict(applied=2, skipped=1)
    # a trainer that has not built its table yet keeps the counters for when it does
    tr3, model3 = _adamw_guarded(dev, init)
    tr3.load_optimizer_state_dict(ck['opt'], ck['sched'])
    assert tr3.iter == 2 and tr3.optimizer_state_dict()['step_guard'] == dict(applied=1, skipped=1)
    # a checkpoint without the entry: every iteration counts as applied
    old = {k: v for k, v in ck['opt'].items() if k != 'step_guard'}
    tr2.load_optimizer_state_dict(old, ck['sched'])
    assert tr2.iter == 2 and tr2.guard.state() == dict(applied=2, skipped=0)
    # a guard-off trainer writes no entry
    assert 'step_guard' not in L.Trainer(model3, _light_cfg()).optimizer_state_dict()


# --------------------------------------------------------------------------- #
# 9. two ranks (gloo, emulator): the pattern of tests/test_clip_grad.py's _w2_worker
# --------------------------------------------------------------------------- #
def _w2_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['LEDN_EXPERIMENTAL'] = '1'
    os.environ['LEDN_MULTI_COMM'] = '1'
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import led_net_amd as L
    from conftest import bind_emu
    import test_step_guard as SG
    cfg = SG._light_cfg()
    img, lab = SG._light_batch(batch=2)
    per = img.shape[0] // world
    img, lab = img[rank * per:(rank + 1) * per], lab[rank * per:(rank + 1) * per]
    samples = [L.SegDataSample(gt=lab[i]) for i in range(per)]
    with bind_emu():
        model = L.MODELS.build(cfg['model'])
        model.load_state_dict(torch.load(os.path.join(out_dir, 'init.pt')))
        tr = L.Trainer(model, cfg, world_size=world, skip_nonfinite=True)
        tr.train_step(img, samples)
        before = {k: v.detach().clone() for k, v in model.state_dict().items() if 'running_' not in k and 'num_batches' not in k}
        tr.forward_backward(img, samples)
        if rank == 1:
            tr.flat_grad[tr.flat_grad.numel() - 2] = NAN          # this rank's gradient only
        out = tr.optimizer_step()
        after = {k: v.detach().clone() for k, v in model.state_dict().items()}
        res = dict(sd=after, unchanged=all(torch.equal(after[k], before[k]) for k in before),
                   finite=float(out['grad_finite']), state=tr.guard.state(), report=tr.nonfinite_report(),
                   grad_max=float(tr.flat_grad.abs().max()))
    torch.save(res, os.path.join(out_dir, f'w2_{rank}.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_world2_a_nan_on_one_rank_makes_both_ranks_skip(tmp_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import led_net_amd as L
    from conftest import bind_emu
    cfg = _light_cfg()
    torch.manual_seed(100)
    with bind_emu():
        model = L.MODELS.build(cfg['model'])
        torch.save({k: v.detach().clone() for k, v in model.state_dict().items()}, tmp_path / 'init.pt')
    port = 37500 + (os.getpid() % 2000)
    ctx = mp.spawn(_w2_worker, args=(2, port, str(tmp_path)), nprocs=2, join=False)
    while not ctx.join():
        pass
    r0 = torch.load(tmp_path / 'w2_0.pt', weights_only=False)
    r1 = torch.load(tmp_path / 'w2_1.pt', weights_only=False)
    for r in (r0, r1):
        assert r['unchanged'] and r['finite'] == 0.0 and r['state'] == dict(applied=1, skipped=1) and r['grad_max'] == 0.0
    assert r0['report'] == r1['report'] and r0['report']['iter'] == 1 and len(r0['report']['params']) == 1
    for k in r0['sd']:
        assert _same(r0['sd'][k], r1['sd'][k]), k


# --------------------------------------------------------------------------- #
# 10. the C ABI
# --------------------------------------------------------------------------- #
def test_entry_points_reject_bad_arguments(emu):
    from led_net_amd import _lib, ops_train as T
    lib = _lib.get_lib().cdll
    assert lib.ledn_abi_version() == 5 == _lib.ABI_VERSION
    for name in ('ledn_grad_finite_pass', 'ledn_step_guard_verdict', 'ledn_optim_step_guarded'):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert C.sizeof(_lib.StepGuardDesc) == 32 and _lib.GUARD_WORDS * 4 == 48
    p, g, m, v = torch.randn(100), torch.randn(100), torch.zeros(100), torch.zeros(100)
    avg = torch.randn(100)
    tab = T.OptimTable([p], [g], [m], [v], avgs=[avg])
    guard = T.StepGuard(torch.device('cpu'), 1)
    gd = guard.desc()
    keep = [x.clone() for x in (p, g, m, v, avg, guard.buf)]

    def desc(**kw):
        d = _lib.OptimDesc()
        d.kind, d.has_v, d.lr_a, d.lr_b, d.momentum, d.eps = _lib.OPTIM_ADAMW, 1, 0.01, 0.0, 0.9, 1e-8
        d.beta1, d.beta2, d.weight_decay, d.grad_scale, d.clip = 0.9, 0.999, 0.01, 1.0, _lib.CLIP_OFF
        for k, val in kw.items():
            setattr(d, k, val)
        return d
    tp, ap = tab.table.data_ptr(), tab.avg_table.data_ptr()

    def finite(table=tp, n=1, max_n=100, guard_=gd):
        return lib.ledn_grad_finite_pass(table, n, max_n, C.byref(guard_) if guard_ is not None else None, None)

    def verdict(table=tp, n=1, max_n=100, guard_=gd, b1=0.9, b2=0.999):
        return lib.ledn_step_guard_verdict(table, n, max_n, C.byref(guard_) if guard_ is not None else None, b1, b2, 0,
                                           None, None)

    def step(table=tp, avgs=ap, n=1, max_n=100, d=None, guard_=gd, w=0.5):
        return lib.ledn_optim_step_guarded(table, avgs, n, max_n, C.byref(d) if d is not None else None,
                                           C.byref(guard_) if guard_ is not None else None, w, None, None)
    hollow = _lib.StepGuardDesc()
    hollow.words, hollow.bad, hollow.flags, hollow.last_bad = gd.words, gd.bad, None, gd.last_bad
    for fn in (finite, verdict, lambda **kw: step(d=desc(), **kw)):
        assert fn(guard_=None) == _lib.EINVAL and fn(guard_=hollow) == _lib.EINVAL
        assert fn(table=None) == _lib.EINVAL
        assert fn(n=0) == _lib.EINVAL and fn(n=-1) == _lib.EINVAL and fn(max_n=0) == _lib.EINVAL
    for kw in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=NAN)):
        assert verdict(**kw) == _lib.EINVAL
    # whatever ledn_optim_step / ledn_optim_step_ema reject
    for kw in (dict(kind=2), dict(beta1=1.0), dict(eps=0.0), dict(has_v=0), dict(clip=3),
               dict(clip=_lib.CLIP_NORM, norm_type=_lib.NORM_L2, n_partials=1, max_norm=1.0),       # partials NULL
               dict(clip=_lib.CLIP_VALUE, clip_value=0.0)):
        assert step(d=desc(**kw)) == _lib.EINVAL, kw
    assert step(d=None) == _lib.EINVAL
    assert step(d=desc(), w=0.0) == _lib.EINVAL and step(d=desc(), w=1.5) == _lib.EINVAL
    for a, b in zip(keep, (p, g, m, v, avg, guard.buf)):
        assert torch.equal(a, b)                           # nothing was launched
    # AdamW without host bias corrections is fine here: they come from the guard words
    assert finite() == _lib.OK and verdict() == _lib.OK and step(d=desc()) == _lib.OK
    assert step(d=desc(), avgs=None, w=0.0) == _lib.OK      # no averaged copy: w is not looked at
    assert guard.state() == dict(applied=1, skipped=0) and not torch.equal(p, keep[0])
