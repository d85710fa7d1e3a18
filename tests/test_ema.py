"""Weight averaging (mmengine EMAHook) folded into the optimizer launch: ledn_optim_step_ema / ledn_ema_update, the
Trainer around them, the checkpoint swap and the command line.  Expected values come from plain torch: Tensor.lerp_ on a
float64 shadow copy.  Emulator on the CPU; the same bodies on the MI355X with -m gpu.

Bound on one update.  avg_new = avg + w * (p - avg) is three f32 roundings (the difference, the product, the sum; an FMA
merges the last two), each at most half an ulp of a quantity bounded by |avg_old| + |p_new| for 0 < w <= 1.  So
    |got - want| <= 2 * eps32 * (|avg_old| + |p_new|)       elementwise, no relative term,
with want the float64 lerp of avg_old towards the p_new the kernel itself wrote and w the f32 value the kernel receives.
Both algebraic forms of the lerp, with or without FMA, stay inside.  Over several steps the Trainer tests sum that bound
over the steps taken (every later update multiplies an earlier error by 1 - w < 1).

Frozen parameter: the issue points at tests/test_train_frozen.py for the set-up, but that file freezes the step's
discrete decisions, not a parameter; here a parameter is frozen with requires_grad_(False) before the Trainer is built,
which is what keeps it out of the optimizer table."""
import copy
import ctypes as C
import math
import os
import subprocess
import sys
import warnings

import pytest
import torch

import test_optim_step as TOS
from conftest import slow_on_emu
from test_optim_step import CFG, HYP, LR_MULTS, ROOT, SIZES, WD_MULTS, _batch, _clip_obj, _kind_id, _off, _table

EMA_CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_ema_config.py')
EPS32 = float(torch.finfo(torch.float32).eps)
_DEV = [torch.device('cpu')]
AVG_OFF = (1, 0, 0, 0, 0, 0, 0)     # tensor 0: p, g, m 16-byte aligned, avg one float off -> the scalar path because of avg alone


@pytest.fixture(autouse=True)
def _track_device(request):
    _DEV[0] = TOS._DEV[0] = request.getfixturevalue('be').dev if 'be' in request.fixturenames else torch.device('cpu')
    yield


def D(t):
    return t.to(_DEV[0])


def f32(w):
    return float(torch.tensor(w, dtype=torch.float32))


def _assert_lerp(got, avg_old, p_new, w, what, steps=1):
    """the module docstring's bound, `steps` times"""
    got, avg_old, p_new = (x.detach().double().cpu().reshape(-1) for x in (got, avg_old, p_new))
    want = avg_old.lerp(p_new, f32(w))
    err, bound = (got - want).abs(), steps * 2 * EPS32 * (avg_old.abs() + p_new.abs())
    print(f'{what}: max |got - want| = {float(err.max()):.3e}, max err / bound = {float((err / (bound + 1e-300)).max()):.3f}')
    bad = ~(err <= bound)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} outside, first at {int(bad.nonzero()[0])}'


def _avgs(seed, sizes=SIZES, off=AVG_OFF, fill=None):
    g = torch.Generator().manual_seed(1000 + seed)
    host = [torch.randn(n, generator=g) if fill is None else torch.full((n,), fill) for n in sizes]
    return host, [_off(n, o, fill=x) for n, o, x in zip(sizes, off, host)]


# --------------------------------------------------------------------------- #
# 1. the kernels, single launch
# --------------------------------------------------------------------------- #
def _step(kind, clip_mode, seed, w=None, ema='host', avg_fill=None, avg_is_p=False):
    """one launch over the table of test_optim_step.py; ema: None (ledn_optim_step), 'host' or 'dev' (w by value / through
    the device float) -> state tensors on the CPU, avg_old, avg"""
    from led_net_amd import ops_train as T
    hp, hg, hm, hv, flat, pd, gd, md, vd = _table(kind, seed=seed, warm=True)
    ha, ad = _avgs(seed, fill=avg_fill)
    assert [x.data_ptr() % 16 for x in (pd[0], gd[0], md[0], ad[0])] == [0, 0, 0, 4] and ad[3].data_ptr() % 16 == 0
    tab = T.OptimTable(pd, gd, md, vd, LR_MULTS, WD_MULTS, avgs=ad if ema else None)
    clip, _ = _clip_obj(clip_mode, flat, hg, 0.5)
    if clip is not None:
        clip.norm_pass(flat)
    kw = {}
    if ema == 'host':
        kw = dict(ema_w=w)
    elif ema == 'dev':
        kw = dict(ema_w=0.123, ema_dev=D(torch.tensor([w], dtype=torch.float32)))       # (the host value must be ignored)
    if avg_is_p:                # the average already equals the parameter this step will write: run it once without EMA
        ref = _step(kind, clip_mode, seed, ema=None)[0]
        for a, p in zip(ad, ref[:len(SIZES)]):
            a.copy_(D(p))
        ha = [a.cpu().clone() for a in ad]
    tab.step(_kind_id(kind), 2e-3, 1e-4, grad_scale=0.5, t=37, clip=clip, **kw, **HYP)
    state = [x.cpu().clone() for x in pd + md + (vd or []) + [flat]]
    return state, ha, [a.cpu().clone() for a in ad]


@pytest.mark.parametrize('clip_mode', ['off', 'l2', 'value'])
@pytest.mark.parametrize('kind', ['SGD', 'AdamW'])
def test_optim_step_ema_single_launch(be, kind, clip_mode):
    w = 0.3
    plain, _, _ = _step(kind, clip_mode, 7, ema=None)
    state, avg_old, avg = _step(kind, clip_mode, 7, w, 'host')
    for i, (a, b) in enumerate(zip(state, plain)):          # p, m, v, g: the bits of ledn_optim_step
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i
    assert float(state[-1].abs().max()) == 0.0
    for i in range(len(SIZES)):
        assert not torch.equal(avg[i], avg_old[i])
        _assert_lerp(avg[i], avg_old[i], state[i], w, f'{kind} {clip_mode} avg[{i}]')
    state_d, _, avg_d = _step(kind, clip_mode, 7, w, 'dev')  # w through the device float: the same bits
    for i, (a, b) in enumerate(zip(state_d + avg_d, state + avg)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i


@pytest.mark.parametrize('ema', ['host', 'dev'])
@pytest.mark.parametrize('fill', [float('nan'), float('inf')])
@pytest.mark.parametrize('kind', ['SGD', 'AdamW'])
def test_optim_step_ema_w1_is_a_copy(be, kind, fill, ema):
    state, _, avg = _step(kind, 'off', 11, 1.0, ema, avg_fill=fill)
    for i in range(len(SIZES)):
        assert torch.equal(avg[i], state[i]), i


@pytest.mark.parametrize('kind', ['SGD', 'AdamW'])
def test_optim_step_ema_equal_average_is_unchanged(be, kind):
    state, avg_old, avg = _step(kind, 'off', 13, 0.5, 'host', avg_is_p=True)
    for i in range(len(SIZES)):
        assert torch.equal(avg_old[i], state[i])            # (the set-up: avg_old == p_new)
        assert torch.equal(avg[i].view(torch.int32), avg_old[i].view(torch.int32)), i


U_SIZES = (1, 3, 4097, 8)
U_AVG_OFF = (0, 0, 0, 1)
U_SRC_OFF = (0, 1, 0, 0)


def _update(w, ema='host', fill=None, same=False):
    from led_net_amd import ops_train as T
    g = torch.Generator().manual_seed(17)
    hs = [torch.randn(n, generator=g) for n in U_SIZES]
    sd = [_off(n, o, fill=x) for n, o, x in zip(U_SIZES, U_SRC_OFF, hs)]
    ha, ad = _avgs(19, U_SIZES, U_AVG_OFF, fill)
    if same:
        for a, x in zip(ad, sd):
            a.copy_(x)
        ha = [x.clone() for x in hs]
    assert ad[2].data_ptr() % 16 == 0 and sd[2].data_ptr() % 16 == 0 and ad[3].data_ptr() % 16 == 4
    tab = T.EmaTable(ad, sd)
    if ema == 'host':
        tab.update(w=w)
    else:
        tab.update(w=0.123, w_dev=D(torch.tensor([w], dtype=torch.float32)))
    for x, h in zip(sd, hs):
        assert torch.equal(x.cpu(), h)                      # the source is only read
    return hs, ha, [a.cpu().clone() for a in ad]


def test_ema_update_single_launch(be):
    from led_net_amd import _lib
    w = 0.3
    res = {}
    for det in (False, True):
        _lib.set_deterministic(det)
        try:
            hs, ha, avg = _update(w)
        finally:
            _lib.set_deterministic(False)
        res[det] = avg
        for i in range(len(U_SIZES)):
            assert not torch.equal(avg[i], ha[i])
            _assert_lerp(avg[i], ha[i], hs[i], w, f'ema_update avg[{i}]')
    _, _, avg_d = _update(w, 'dev')
    for i in range(len(U_SIZES)):                           # either determinism mode, w by value or from the device
        assert torch.equal(res[False][i].view(torch.int32), res[True][i].view(torch.int32))
        assert torch.equal(res[False][i].view(torch.int32), avg_d[i].view(torch.int32))
    for fill in (float('nan'), float('inf')):               # w = 1: a copy, whatever the average held
        for ema in ('host', 'dev'):
            hs, _, avg = _update(1.0, ema, fill=fill)
            assert all(torch.equal(a, s) for a, s in zip(avg, hs))
    hs, ha, avg = _update(0.5, same=True)                   # avg_old == src: bit-unchanged
    assert all(torch.equal(a.view(torch.int32), h.view(torch.int32)) for a, h in zip(avg, ha))


def test_ema_entry_points_reject_bad_arguments(emu):
    from led_net_amd import _lib, ops_train as T
    lib = _lib.get_lib().cdll
    p, g, m, a = torch.randn(100), torch.randn(100), torch.zeros(100), torch.randn(100)
    p0, a0 = p.clone(), a.clone()
    tab, upd = T.OptimTable([p], [g], [m], avgs=[a]), T.EmaTable([a], [p])
    wdev = torch.tensor([0.5])
    d = _lib.OptimDesc()
    d.kind, d.lr_a, d.momentum, d.grad_scale, d.clip = _lib.OPTIM_SGD, 0.01, 0.9, 1.0, _lib.CLIP_OFF

    def step(table=tab.table.data_ptr(), avgs=tab.avg_table.data_ptr(), n=1, max_n=100, desc=C.byref(d), w=0.5, w_dev=None):
        return lib.ledn_optim_step_ema(table, avgs, n, max_n, desc, w, w_dev, None)

    def update(table=upd.table.data_ptr(), n=1, max_n=100, w=0.5, w_dev=None):
        return lib.ledn_ema_update(table, n, max_n, w, w_dev, None)
    for w in (0.0, -0.1, 1.5, float('nan'), float('inf')):
        assert step(w=w) == _lib.EINVAL and update(w=w) == _lib.EINVAL, w
    assert step(table=None) == _lib.EINVAL and step(avgs=None) == _lib.EINVAL and step(desc=None) == _lib.EINVAL
    assert step(n=0) == _lib.EINVAL and step(max_n=0) == _lib.EINVAL
    assert update(table=None) == _lib.EINVAL and update(n=0) == _lib.EINVAL and update(max_n=0) == _lib.EINVAL
    d.clip = 7
    assert step() == _lib.EINVAL                            # what ledn_optim_step rejects
    d.clip = _lib.CLIP_OFF
    assert torch.equal(p, p0) and torch.equal(a, a0)        # nothing was launched
    assert step(w=7.0, w_dev=wdev.data_ptr()) == _lib.OK and update(w=-1.0, w_dev=wdev.data_ptr()) == _lib.OK
    assert step(w=1.0) == _lib.OK and update(w=1.0) == _lib.OK and torch.equal(a, p)
    assert C.sizeof(_lib.EmaEntry) == 24 and C.sizeof(_lib.OptimEntry) == 48
    with pytest.raises(_lib.LednError):
        tab.step(_lib.OPTIM_SGD, 0.01)                      # a table with avgs needs the weight
    with pytest.raises(_lib.LednError):
        T.OptimTable([p], [g], [m]).step(_lib.OPTIM_SGD, 0.01, ema_w=0.5)
    with pytest.raises(_lib.LednError):
        T.OptimTable([p], [g], [m], avgs=[a, a])
    with pytest.raises(_lib.LednError):
        T.EmaTable([a], [torch.randn(99)])
    with pytest.raises(_lib.LednError):
        upd.update()


# --------------------------------------------------------------------------- #
# 2. the hook's configuration
# --------------------------------------------------------------------------- #
def test_parse_ema_hook():
    from led_net_amd import optim as O
    assert O.parse_ema_hook(None) is None and O.parse_ema_hook([]) is None
    assert O.parse_ema_hook([dict(type='SegVisualizationHook', draw=True)]) is None         # other hooks: not ours
    assert O.parse_ema_hook([dict(type='Other'), dict(type='EMAHook')]) == dict(
        ema_type='ExponentialMovingAverage', momentum=0.0002, gamma=None, update_buffers=False, begin_iter=0)
    got = O.parse_ema_hook([dict(type='EMAHook', ema_type='ExpMomentumEMA', momentum=0.01, update_buffers=True, begin_iter=4,
                                 interval=1, priority='NORMAL')])
    assert got == dict(ema_type='ExpMomentumEMA', momentum=0.01, gamma=2000, update_buffers=True, begin_iter=4)
    assert O.ema_weight(got, 5) == (1 - 0.01) * math.exp(-6 / 2000) + 0.01


@pytest.mark.parametrize('bad,word', [
    (dict(strict_load=False), 'strict_load'), (dict(begin_epoch=1), 'begin_epoch'), (dict(interval=2), 'interval'),
    (dict(ema_type='StochasticWeightAverage'), 'ema_type'), (dict(momentum=0.0), 'momentum'), (dict(momentum=1.0), 'momentum'),
    (dict(momentum=-0.1), 'momentum'), (dict(momentum='0.1'), 'momentum'), (dict(gamma=100), 'gamma'),
    (dict(ema_type='ExpMomentumEMA', gamma=0), 'gamma'), (dict(begin_iter=-1), 'begin_iter'), (dict(device='cpu'), 'device')])
def test_bad_ema_hook_raises_value_error(bad, word):
    import led_net_amd as L
    from led_net_amd import optim as O
    with pytest.raises(ValueError, match=word):
        O.parse_ema_hook([dict(type='EMAHook', **bad)])
    if word in ('strict_load', 'interval'):                 # ... and through the config, where the Trainer reads it
        cfg = L.load_config(EMA_CFG)
        cfg['custom_hooks'] = [dict(type='EMAHook', **bad)]
        with pytest.raises(ValueError, match=word):
            L.Trainer(L.MODELS.build(cfg['model']), cfg)
    with pytest.raises(ValueError, match='more than one'):
        O.parse_ema_hook([dict(type='EMAHook'), dict(type='EMAHook', momentum=0.5)])


# --------------------------------------------------------------------------- #
# 3. the Trainer
# --------------------------------------------------------------------------- #
FROZEN = 'backbone.stem.0.conv.weight'
STEPS = 6


def _full(dev):
    """A step of the whole network takes ~35 s on the CPU emulator.  Every test of this section has a -m gpu twin (the
    same body on the MI355X) that always runs in full; on the emulator the default run keeps one two-step case (the
    first-step copy, one lerp, the frozen parameter, the running statistics, the swap) and LEDN_EMU_SLOW=1 runs all."""
    return dev.type != 'cpu' or bool(int(os.environ.get('LEDN_EMU_SLOW', '0')))


def _trainer(dev, hook, seed=304, freeze=None, init=None, via_cfg=False, **kw):
    """the tiny SGD / PolyLR configuration of the other Trainer tests (+ an EMAHook); hook: the hook's keys or None"""
    import led_net_amd as L
    from led_net_amd import optim as O
    torch.manual_seed(seed)
    cfg = L.load_config(CFG)
    for c in cfg['model']['decode_head']['loss_decode']:
        c['min_kept'] = 20000
    model = L.MODELS.build(cfg['model'])
    if init is not None:
        model.load_state_dict(init)
    model.to(dev)
    if freeze:
        dict(model.named_parameters())[freeze].requires_grad_(False)
    hooks = [dict(type='EMAHook', **hook)] if hook is not None else None
    if via_cfg:
        cfg['custom_hooks'] = hooks
        return L.Trainer(model, cfg, max_iters=50, **kw), model
    return L.Trainer(model, cfg, max_iters=50, ema=O.parse_ema_hook(hooks), **kw), model


def _averaged(tr):
    """name -> (the model's tensor, the trainer's averaged view)"""
    return {name: (t, a) for name, t, a in tr._ema_named()}


class _Shadow:
    """the issue's rule in float64, advanced from the trainer's own current tensors after every step; `bound` sums the
    single-update bound (module docstring) over the lerp steps taken"""

    def __init__(self, hook):
        self.hook, self.steps, self.avg, self.bound, self.ws = hook, 0, {}, {}, []

    def step(self, it, current):
        h = self.hook
        copy_ = it < h.get('begin_iter', 0) or self.steps == 0
        if not copy_:
            w = h['momentum']
            if h.get('ema_type') == 'ExpMomentumEMA':
                w = (1 - h['momentum']) * math.exp(-(1 + self.steps) / h['gamma']) + h['momentum']
            self.ws.append(w)
        for k, t in current.items():
            t = t.detach().double().cpu()
            if copy_:
                self.avg[k], self.bound[k] = t.clone(), torch.zeros_like(t)
            else:
                self.bound[k] += 2 * EPS32 * (self.avg[k].abs() + t.abs())
                self.avg[k].lerp_(t, f32(w))
        if it >= h.get('begin_iter', 0):
            self.steps += 1
        return copy_


@pytest.mark.parametrize('hook', [dict(momentum=0.1, update_buffers=True),
                                  dict(ema_type='ExpMomentumEMA', momentum=0.01, gamma=3),
                                  dict(momentum=0.1, begin_iter=3)], ids=['buffers', 'expmomentum', 'begin_iter'])
def test_trainer_average_follows_the_rule(be, hook):
    if 'update_buffers' not in hook:
        slow_on_emu(be.dev)
    steps = STEPS if _full(be.dev) else 2                   # (the emulator's default run: the copy and one lerp)
    tr, model = _trainer(be.dev, hook, freeze=FROZEN, via_cfg='gamma' in hook)
    batch = _batch(be.dev, batch=1)
    shadow, worst = _Shadow(hook), 0.0
    for it in range(steps):
        tr.train_step(*batch)
        av = _averaged(tr)
        copied = shadow.step(it, {k: t for k, (t, a) in av.items()})
        assert tr.ema_steps == shadow.steps and tr.iter == it + 1
        moved = 0
        for k, (t, a) in av.items():
            if copied:                                      # the first update, and everything before begin_iter
                assert torch.equal(a, t), (it, k)
                continue
            err = (a.detach().double().cpu() - shadow.avg[k]).abs()
            assert bool((err <= shadow.bound[k]).all()), (it, k, float(err.max()), float(shadow.bound[k].max()))
            worst = max(worst, float((err / (shadow.bound[k] + 1e-300)).max()))
            moved += int(not torch.equal(a, t))
        assert copied == (it == 0 if 'begin_iter' not in hook else it <= 3), it
        assert copied or moved > 100                        # a lerp step leaves the average behind the parameters
    print(f'{hook}: worst err / bound over {steps} steps = {worst:.3f}, weights {shadow.ws}')
    av = _averaged(tr)
    assert FROZEN in av and torch.equal(av[FROZEN][1], av[FROZEN][0]) and FROZEN not in set(tr.names)
    assert len(av) == len(list(model.parameters())) + (sum(b.is_floating_point() for b in model.buffers())
                                                       if hook.get('update_buffers') else 0)
    if 'gamma' in hook:
        assert len(shadow.ws) == STEPS - 1 and len(set(shadow.ws)) == len(shadow.ws)     # a new weight every step
    if hook.get('update_buffers'):
        rm = [k for k in av if k.endswith('running_mean')]
        assert rm and any(not torch.equal(av[k][1], av[k][0]) for k in rm)
        avg = tr.ema_state()['state_dict']
        with tr.ema_weights():                              # the averaged model has its own running statistics
            sd = model.state_dict()
            assert all(torch.equal(sd[k].cpu(), avg[k]) for k in sd)
            assert any(not torch.equal(sd[k], av[k][1]) for k in rm)        # (the views now hold the training model's)
        assert all(torch.equal(v, av[k][0]) for k, v in model.state_dict().items() if k in av)


def test_trainer_ema_leaves_training_alone_and_swaps(be):
    import led_net_amd as L
    slow_on_emu(be.dev)
    L.set_deterministic(True)
    try:
        _, m0 = _trainer(be.dev, None)
        init = copy.deepcopy(m0.state_dict())
        batch = _batch(be.dev, batch=1)
        runs = []
        for hook in (None, dict(momentum=0.1)):
            tr, model = _trainer(be.dev, hook, init=init)
            assert (tr.ema is None) == (hook is None) and tr._general == (hook is not None)
            for _ in range(STEPS):
                tr.train_step(*batch)
            runs.append((tr, model))
        (plain, mp), (tr, model) = runs
        assert type(plain.table).__name__ == 'SgdTable' and plain.flat_ema is None and plain._ema_dev is None
        assert type(tr.table).__name__ == 'OptimTable' and tr.table.avgs is not None
        bad = [k for k, v in mp.state_dict().items() if not torch.equal(v, model.state_dict()[k])]
        assert not bad, bad[:5]                             # the hook changes nothing the training computes
        assert torch.equal(plain.flat_mom, tr.flat_mom)
    finally:
        L.set_deterministic(False)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    avg = tr.ema_state()['state_dict']
    img = batch[0]
    with tr.ema_weights() as m:
        assert m is model
        inside = {k: v.detach().clone() for k, v in model.state_dict().items()}
        model.eval()
        with torch.no_grad():
            out = model(img, mode='predict')
        model.train()
        assert torch.isfinite(out[0].seg_logits.data.float()).all()
    assert set(avg) == set(before)
    n_diff = 0
    for k in before:
        assert torch.equal(inside[k].cpu(), avg[k]), k
        if 'running_' in k or 'num_batches' in k:
            assert torch.equal(inside[k], before[k]), k     # update_buffers=False: the buffers are the training model's
        else:
            n_diff += int(not torch.equal(inside[k], before[k]))
    assert n_diff > 100
    after = model.state_dict()
    assert all(torch.equal(after[k], before[k]) for k in before)            # swapped back bit-exactly
    assert all(torch.equal(tr.ema_state()['state_dict'][k], avg[k]) for k in avg)


# --------------------------------------------------------------------------- #
# 4. the graph (GPU only): w and the copy decision are read at replay time
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
def test_replay_equals_eager_with_expmomentum_and_begin_iter():
    import led_net_amd as L
    dev = torch.device('cuda:0')
    TOS._DEV[0] = _DEV[0] = dev
    hook = dict(ema_type='ExpMomentumEMA', momentum=0.01, gamma=3, begin_iter=2)
    L.set_deterministic(True)
    try:
        _, m0 = _trainer(dev, None)
        init = copy.deepcopy(m0.state_dict())
        batches = [_batch(dev, seed=31 + k, batch=1) for k in range(5)]
        res = []
        for graph in (False, True):
            tr, model = _trainer(dev, hook, init=init)
            if graph:
                tr.capture(*batches[0], warmup=2, restore=True)
                assert tr.iter == 0 and tr.ema_steps == 0
                assert all(torch.equal(a, t) for _, t, a in tr._ema_named())
            else:
                snap = ([p.detach().clone() for p in tr.params], [b.detach().clone() for b in model.buffers()],
                        tr.flat_mom.clone(), tr.flat_ema.clone())
                for _ in range(2):                          # the same warm-up the capture runs, put back the same way
                    tr.train_step(*batches[0])
                with torch.no_grad():
                    for p, v in zip(tr.params, snap[0]):
                        p.copy_(v)
                    for b, v in zip(model.buffers(), snap[1]):
                        b.copy_(v)
                    tr.flat_mom.copy_(snap[2])
                    tr.flat_ema.copy_(snap[3])
                tr.iter, tr.ema_steps = 0, 0
            ws = []
            for b in batches:
                ws.append(tr._ema_w())
                tr.replay(*b) if graph else tr.train_step(*b)
            torch.cuda.synchronize()
            assert ws[:3] == [1.0, 1.0, 1.0] and 0.01 < ws[4] < ws[3] < 1.0 and tr.ema_steps == 3
            res.append(({k: v.detach().clone() for k, v in model.state_dict().items()}, tr.flat_ema.clone(), tr.flat_mom.clone()))
        (sd_e, ema_e, mom_e), (sd_g, ema_g, mom_g) = res
        bad = [k for k in sd_e if not torch.equal(sd_e[k], sd_g[k])]
        assert not bad, bad[:5]
        assert torch.equal(mom_e, mom_g) and torch.equal(ema_e, ema_g)
        assert not torch.equal(ema_e[:tr.flat_mom.numel()], torch.cat([p.detach().reshape(-1) for p in tr.params]))
    finally:
        L.set_deterministic(False)


# --------------------------------------------------------------------------- #
# 5. the checkpoint
# --------------------------------------------------------------------------- #
def test_checkpoint_swap_and_resume(be, tmp_path):
    import led_net_amd as L
    slow_on_emu(be.dev)
    dev, hook = be.dev, dict(momentum=0.1)
    L.set_deterministic(True)
    try:
        _, m0 = _trainer(dev, None)
        init = copy.deepcopy(m0.state_dict())
        batches = [_batch(dev, seed=41 + k, batch=1) for k in range(5)]
        tr, model = _trainer(dev, hook, init=init)
        for b in batches[:3]:
            tr.train_step(*b)
        path = str(tmp_path / 'iter_3.pth')
        L.save_checkpoint(model, path, meta=dict(iter=3), trainer=tr)
        ck = torch.load(path, weights_only=False)
        sd, avg = model.state_dict(), tr.ema_state()['state_dict']
        assert list(ck['state_dict']) == list(sd)           # the key set (and order) of state_dict is unchanged
        es = ck['ema_state_dict']
        assert es['steps'].dtype == torch.int64 and es['steps'].ndim == 0 and int(es['steps']) == 3
        assert set(es) == {'steps'} | {'module.' + k for k in sd}
        n_diff = 0
        for k, v in sd.items():
            assert torch.equal(ck['state_dict'][k], avg[k]) and torch.equal(es['module.' + k], v.cpu()), k
            n_diff += int(not torch.equal(avg[k], v.cpu()))
        assert n_diff > 100                                 # ... and the two really are different weights
        # a fresh model and Trainer resume: parameters, average, counter; then two more steps = the uninterrupted run's
        tb, mb = _trainer(dev, hook, seed=999)
        ckb = L.load_checkpoint(mb, path)
        assert all(torch.equal(v.cpu(), avg[k]) for k, v in mb.state_dict().items())     # (what a plain load sees)
        L.resume(tb, ckb)
        assert tb.iter == 3 and tb.ema_steps == 3 and tb.lr() == tr.lr()
        assert all(torch.equal(v, sd[k]) for k, v in mb.state_dict().items())
        assert all(torch.equal(v, avg[k]) for k, v in tb.ema_state()['state_dict'].items())
        pa, pb = {id(p): i for i, p in enumerate(tr.params)}, {id(p): i for i, p in enumerate(tb.params)}
        for p_a, p_b in zip(model.parameters(), mb.parameters()):
            assert torch.equal(tr.moms[pa[id(p_a)]], tb.moms[pb[id(p_b)]])
        more = batches[3:]
        for t_ in (tr, tb):
            for b in more:
                t_.train_step(*b)
        assert tb.ema_steps == tr.ema_steps == 3 + len(more)
        bad = [k for k, v in model.state_dict().items() if not torch.equal(v, mb.state_dict()[k])]
        assert not bad, bad[:5]
        assert torch.equal(tr.flat_ema, tb.flat_ema) and torch.equal(tr.flat_mom, tb.flat_mom)
    finally:
        L.set_deterministic(False)
    # init_model evaluates the averaged weights with no flag
    cfg = L.load_config(CFG)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = L.init_model(cfg, path, device=dev)
    assert all(torch.equal(v.cpu(), avg[k]) for k, v in m.state_dict().items())
    # a checkpoint without the key, loaded into an EMA run: a warning, and the average starts from the loaded weights
    plain_path = str(tmp_path / 'plain.pth')
    tp, mp = _trainer(dev, None, init=init)
    L.save_checkpoint(mp, plain_path, meta=dict(iter=0), trainer=tp)
    assert 'ema_state_dict' not in torch.load(plain_path, weights_only=False)
    tc, mc = _trainer(dev, hook, seed=5)
    tc.ema_steps = 7
    ckc = L.load_checkpoint(mc, plain_path)
    with pytest.warns(UserWarning, match='ema_state_dict'):
        L.resume(tc, ckc)
    assert tc.ema_steps == 0 and all(torch.equal(a, t) for _, t, a in tc._ema_named())
    assert all(torch.equal(v.cpu(), init[k].cpu()) for k, v in mc.state_dict().items())


# --------------------------------------------------------------------------- #
# 6. the command line
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
def test_train_cli_writes_the_ema_checkpoint(tmp_path):
    def run(extra, wd):
        env = dict(os.environ, PYTHONPATH=ROOT)
        args = [sys.executable, 'tools/train.py', EMA_CFG, '--max-iters', '3', '--batch-size', '2', '--height', '320',
                '--width', '320', '--f32', '--work-dir', str(tmp_path / wd)] + extra
        r = subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, f'{args}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
        return torch.load(str(tmp_path / wd / 'iter_3.pth'), weights_only=False)
    ck = run([], 'ema')
    es = ck['ema_state_dict']
    assert int(es['steps']) == 3 and set(es) == {'steps'} | {'module.' + k for k in ck['state_dict']}
    assert sum(not torch.equal(v, es['module.' + k]) for k, v in ck['state_dict'].items()) > 100
    plain = run(['--cfg-options', 'custom_hooks=[]'], 'plain')
    assert 'ema_state_dict' not in plain and list(plain['state_dict']) == list(ck['state_dict'])
    hook = run(['--cfg-options', "custom_hooks=[{'type':'EMAHook','momentum':0.001,'begin_iter':5}]"], 'late')
    assert int(hook['ema_state_dict']['steps']) == 0
    assert all(torch.equal(v, hook['ema_state_dict']['module.' + k]) for k, v in hook['state_dict'].items())
