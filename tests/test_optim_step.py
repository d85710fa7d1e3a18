"""The generalised optimizer step (ledn_optim_step): SGD / AdamW with per-tensor learning-rate and weight-decay multipliers
(optim_wrapper.paramwise_cfg), the scheduler list collapsed to two scalars, clipping folded in; the Trainer around it,
the checkpoint layout and the config / command-line path.  Expected values come from torch itself (torch.optim.SGD /
torch.optim.AdamW with explicit param groups, clip_grad_norm_ / clip_grad_value_, torch.optim.lr_scheduler).
Emulator on the CPU; the same bodies on the MI355X with -m gpu.

Tolerances.  rtol = 1e-5 is the project's figure for this family (tests/test_clip_grad.py).  It is applied to the UPDATE
p_new - p_old and to the optimizer states.  What is compared are f32 values whose last rounding is not the kernel's to
choose, so every comparison carries an absolute term from the f32 format (eps = 2^-23) and the magnitude of the operands of
the last operation, never from what the kernel returns:
  update   p_new is rounded to f32 by both sides (half an ulp of p each), and AdamW rounds p * (1 - lr*wd) before (another
           half ulp each): 2 * eps * |p_old|.  The update is (a multiple of) the new first moment, whose own rounding
           error (next line) does not shrink when its two terms cancel, so it enters scaled like the moment itself:
           SGD lr * 4 * eps * (|m_old| + |g'| + wd * |p|), AdamW (lr / bc1) / (sqrt(v) / sqrt(bc2) + eps) * 4 * eps *
           (|m_old| + |g'|), with torch's v.  |d_got - d_want| <= rtol * |d_want| + the two terms  (_update_scale)
  m        a sum of two rounded products that may cancel: rtol * |want| + 4 * eps * (|term1| + |term2|)
  v        a sum of non-negative terms, no cancellation: rtol alone (atol 1e-30 for squares that underflow)
The torch side of the single-step and whole-step comparisons runs in float64 on the f32 inputs: torch's own f32
clip_grad_norm_ on the CPU is 1.3e-5 away from the float64 norm over the 1.1M-element table used here (measured; the norm
pass under test is 4e-10 away), which alone would use up the tolerance.  The trajectory test compares against both."""
import copy
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import slow_on_emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_test_config.py')
_DEV = [torch.device('cpu')]
EPS32 = float(torch.finfo(torch.float32).eps)
RTOL = 1e-5


@pytest.fixture(autouse=True)
def _track_device(request):
    _DEV[0] = request.getfixturevalue('be').dev if 'be' in request.fixturenames else torch.device('cpu')
    yield


def D(t):
    return t.to(_DEV[0])


def _assert_within(got, want, scale, what, rtol=RTOL, k=4.0):
    """|got - want| <= rtol * |want| + k * eps32 * scale, elementwise, in float64; NaN must match NaN"""
    got, want, scale = (x.detach().double().cpu().reshape(-1) for x in (got, want, scale))
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what
    ok = torch.isnan(want) | ((got - want).abs() <= rtol * want.abs() + k * EPS32 * scale + 1e-30)
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        raise AssertionError(f'{what}: element {i}: got {float(got[i])!r}, want {float(want[i])!r}, scale {float(scale[i])!r}; '
                             f'{int((~ok).sum())} of {ok.numel()} outside')


def _update_scale(kind, p0, m0, g_used, lr, wd, v_want=None, t=1):
    """the magnitude that 2 * eps multiplies in the bound on the update (module docstring)"""
    p0, m0, g_used = p0.double().cpu(), m0.double().cpu(), g_used.double().cpu()
    if kind == 'AdamW':
        b1, b2 = HYP['betas']
        denom = v_want.double().cpu().sqrt() / math.sqrt(1.0 - b2 ** t) + HYP['eps']
        return p0.abs() + 2.0 * (lr / (1.0 - b1 ** t)) * (m0.abs() + g_used.abs()) / denom
    return p0.abs() + 2.0 * lr * (m0.abs() + g_used.abs() + wd * p0.abs())


# --------------------------------------------------------------------------- #
# 1. the kernel, single step
# --------------------------------------------------------------------------- #
# element counts of the table's tensors, laid out back to back in ONE flat gradient buffer: 4100 and 4097 start 16-byte
# aligned (float4 path, the second with a one-float tail), the others do not (scalar path); 1, 3 and > 1M elements
SIZES = (4100, 1, 3, 4097, 1_100_003, 8, 1000)
P_OFF = (0, 0, 0, 0, 0, 1, 0)              # tensor 5: an aligned gradient next to a parameter one float off alignment
LR_MULTS = (1.0, 0.0, 10.0, 0.5, 1.0, 2.0, 1.0)
WD_MULTS = (1.0, 1.0, 0.0, 0.0, 1.0, 0.5, 3.0)


def _off(n, off, gen=None, fill=None):
    base = torch.zeros(n + 4, device=_DEV[0])
    assert base.data_ptr() % 16 == 0
    t = base[off:off + n]
    if fill is not None:
        t.copy_(D(fill))
    return t


def _table(kind, seed, sizes=SIZES, p_off=P_OFF, warm=False):
    """host values + device tensors of a table; warm: non-zero optimizer states (a step in the middle of a run)"""
    g = torch.Generator().manual_seed(seed)
    hp = [torch.randn(n, generator=g) for n in sizes]
    hg = [torch.randn(n, generator=g) * (0.1 + i) for i, n in enumerate(sizes)]
    hm = [torch.randn(n, generator=g) * 0.1 if warm else torch.zeros(n) for n in sizes]
    hv = [torch.rand(n, generator=g) * 0.01 if warm else torch.zeros(n) for n in sizes]
    flat = torch.zeros(sum(sizes) + 4, device=_DEV[0])[:sum(sizes)]
    gd, o = [], 0
    for n, x in zip(sizes, hg):
        gd.append(flat[o:o + n])
        gd[-1].copy_(D(x))
        o += n
    pd = [_off(n, po, fill=x) for n, po, x in zip(sizes, p_off, hp)]
    md = [_off(n, 0, fill=x) for n, x in zip(sizes, hm)]
    vd = [_off(n, 0, fill=x) for n, x in zip(sizes, hv)] if kind == 'AdamW' else None
    return hp, hg, hm, hv, flat, pd, gd, md, vd


HYP = dict(momentum=0.9, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)


def _clip_obj(mode, flat, hg, grad_scale):
    from led_net_amd import _lib, ops_train as T
    if mode == 'off':
        return None, None
    if mode == 'value':
        return T.GradClip(_DEV[0], flat.numel(), norm_type=_lib.NORM_NONE, clip_value=0.7), 0.7
    p_ = 2.0 if mode == 'l2' else math.inf
    total = float(torch.linalg.vector_norm(torch.cat(hg).double() * grad_scale, p_))
    nt = _lib.NORM_L2 if mode == 'l2' else _lib.NORM_INF
    return T.GradClip(_DEV[0], flat.numel(), norm_type=nt, max_norm=0.5 * total), 0.5 * total


def _torch_step(kind, hp, hg, hm, hv, lrs, wds, t, clip_mode, clip_arg, grad_scale, dtype=torch.float64):
    ref = [p.clone().to(dtype).requires_grad_(True) for p in hp]
    groups = [dict(params=[r_], lr=lr, weight_decay=wd) for r_, lr, wd in zip(ref, lrs, wds)]
    if kind == 'AdamW':
        opt = torch.optim.AdamW(groups, betas=HYP['betas'], eps=HYP['eps'])
    else:
        opt = torch.optim.SGD(groups, momentum=HYP['momentum'])
    for r_, m, v in zip(ref, hm, hv):
        if kind == 'AdamW':
            opt.state[r_] = {'step': torch.tensor(float(t - 1)), 'exp_avg': m.clone().to(dtype), 'exp_avg_sq': v.clone().to(dtype)}
        elif t > 1:
            opt.state[r_] = {'momentum_buffer': m.clone().to(dtype)}
    for r_, g in zip(ref, hg):
        r_.grad = (g.to(dtype) * grad_scale)
    norm = None
    if clip_mode == 'value':
        torch.nn.utils.clip_grad_value_(ref, clip_arg)
    elif clip_mode != 'off':
        norm = torch.nn.utils.clip_grad_norm_(ref, clip_arg, norm_type=2.0 if clip_mode == 'l2' else math.inf)
    used = [r_.grad.clone() for r_ in ref]
    opt.step()
    if kind == 'AdamW':
        ms, vs = [opt.state[r_]['exp_avg'] for r_ in ref], [opt.state[r_]['exp_avg_sq'] for r_ in ref]
    else:
        ms, vs = [opt.state[r_]['momentum_buffer'] for r_ in ref], None
    return [r_.detach() for r_ in ref], ms, vs, used, norm


def _kind_id(kind):
    from led_net_amd import _lib
    return _lib.OPTIM_ADAMW if kind == 'AdamW' else _lib.OPTIM_SGD


@pytest.mark.parametrize('t,A,B', [(1, 3e-3, 0.0), (1000, 2e-3, 1e-4)])
@pytest.mark.parametrize('clip_mode', ['off', 'l2', 'inf', 'value'])
@pytest.mark.parametrize('kind', ['SGD', 'AdamW'])
def test_single_step_vs_torch(be, kind, clip_mode, t, A, B):
    from led_net_amd import ops_train as T
    grad_scale = 0.5
    hp, hg, hm, hv, flat, pd, gd, md, vd = _table(kind, seed=t, warm=t > 1)
    assert [x.data_ptr() % 16 for x in gd][:4] == [0, 0, 4, 0] and pd[5].data_ptr() % 16 == 4
    tab = T.OptimTable(pd, gd, md, vd, LR_MULTS, WD_MULTS)
    clip, clip_arg = _clip_obj(clip_mode, flat, hg, grad_scale)
    if clip is not None:
        clip.norm_pass(flat)
    tab.step(_kind_id(kind), A, B, grad_scale=grad_scale, t=t, clip=clip, **HYP)
    lrs = [lm * A + B for lm in LR_MULTS]
    wds = [wm * HYP['weight_decay'] for wm in WD_MULTS]
    want_p, want_m, want_v, used, norm = _torch_step(kind, hp, hg, hm, hv, lrs, wds, t, clip_mode, clip_arg, grad_scale)
    if norm is not None:
        torch.testing.assert_close(clip.total_norm.cpu(), norm.float(), rtol=RTOL, atol=0)
        assert float(clip.coef) < 1.0
    assert float(flat.abs().max()) == 0.0                                   # gradients re-zeroed
    for i in range(len(SIZES)):
        p0 = hp[i]
        scale = _update_scale(kind, p0, hm[i], used[i], lrs[i], wds[i], want_v[i] if kind == 'AdamW' else None, t)
        _assert_within(pd[i].cpu().double() - p0.double(), want_p[i].double() - p0.double(), scale, f'update[{i}]', k=2.0)
        if kind == 'AdamW':
            _assert_within(md[i], want_m[i], hm[i].abs() + used[i].abs(), f'exp_avg[{i}]')
            torch.testing.assert_close(vd[i].cpu().double(), want_v[i], rtol=RTOL, atol=1e-30)
        else:
            _assert_within(md[i], want_m[i], hm[i].abs() + used[i].abs() + wds[i] * p0.abs(), f'momentum[{i}]')
    moved = [not torch.equal(pd[i].cpu(), hp[i]) for i in range(len(SIZES))]
    assert moved == [lr != 0.0 for lr in lrs]                               # lr_mult 0: only B moves that tensor


@pytest.mark.parametrize('clip_mode', ['off', 'l2', 'inf', 'value'])
def test_neutral_sgd_form_is_bit_identical_to_ledn_sgd_step(be, clip_mode):
    """every multiplier 1 and B = 0: the bits of ledn_sgd_step (ledn_sgd_step_clip when clipping), over two steps"""
    from led_net_amd import _lib, ops_train as T
    res = []
    for general in (False, True):
        hp, hg, hm, hv, flat, pd, gd, md, _ = _table('SGD', seed=5)
        tab = T.OptimTable(pd, gd, md) if general else T.SgdTable(pd, gd, md)
        clip, _ = _clip_obj(clip_mode, flat, hg, 0.5)
        for it in range(2):
            for g, g0 in zip(gd, hg):
                g.copy_(D(g0 * (it + 1)))
            if clip is not None:
                clip.norm_pass(flat)
            if general:
                tab.step(_lib.OPTIM_SGD, 0.01, 0.0, momentum=0.9, weight_decay=5e-4, grad_scale=0.5, clip=clip)
            else:
                tab.step(0.01, 0.9, 5e-4, 0.5, clip=clip)
        res.append([x.cpu() for x in pd + md])
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i


@pytest.mark.parametrize('kind', ['SGD', 'AdamW'])
def test_two_runs_are_bit_identical_and_sched_dev_equals_host_scalars(be, kind):
    """no atomics: the same bits on every run with deterministic mode off; the four scalars read from the device vector
    give the bits of the same scalars passed by value"""
    from led_net_amd import _lib, ops_train as T
    assert not _lib.is_deterministic()
    res = []
    for run in range(3):
        hp, hg, hm, hv, flat, pd, gd, md, vd = _table(kind, seed=9, warm=True)
        tab = T.OptimTable(pd, gd, md, vd, LR_MULTS, WD_MULTS)
        clip, _ = _clip_obj('l2', flat, hg, 1.0)
        clip.norm_pass(flat)
        dev = None
        A, B, t = 2e-3, 1e-4, 37
        if run == 2:
            dev = D(torch.tensor(T.optim_scalars(A, B, HYP['betas'], t), dtype=torch.float32))
            A, B, t = 123.0, 456.0, 1                                      # (must be ignored)
        tab.step(_kind_id(kind), A, B, t=t, sched_dev=dev, clip=clip, **HYP)
        res.append([x.cpu() for x in pd + md + (vd or [])])
    for other in res[1:]:
        for i, (a, b) in enumerate(zip(res[0], other)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i


@pytest.mark.parametrize('kind', ['SGD', 'AdamW'])
def test_nan_gradients_propagate(be, kind):
    from led_net_amd import ops_train as T
    sizes, off = (8, 4100), (1, 0)          # scalar path (parameter off alignment) and float4 path
    for clip_mode in ('off', 'value', 'l2'):
        hp, hg, hm, hv, flat, pd, gd, md, vd = _table(kind, seed=3, sizes=sizes, p_off=off)
        gd[0][2] = float('nan')
        gd[1][4099] = float('nan')
        clip, _ = _clip_obj(clip_mode, flat, hg, 1.0)
        if clip is not None:
            clip.norm_pass(flat)
        T.OptimTable(pd, gd, md, vd).step(_kind_id(kind), 1e-2, 0.0, clip=clip, **HYP)
        for p, m, pos in ((pd[0], md[0], 2), (pd[1], md[1], 4099)):
            assert math.isnan(float(p[pos])) and math.isnan(float(m[pos])), (clip_mode, pos)
            n_nan = int(torch.isnan(p).sum())
            assert n_nan == (p.numel() if clip_mode == 'l2' else 1), (clip_mode, n_nan)   # a NaN norm reaches everything
        assert float(flat.abs().max()) == 0.0


def test_entry_point_rejects_bad_arguments(emu):
    from led_net_amd import _lib, ops_train as T
    lib = _lib.get_lib().cdll
    p, g, m, v = torch.randn(100), torch.randn(100), torch.zeros(100), torch.zeros(100)
    part = torch.zeros(256 + 2)
    tab_v, tab = T.OptimTable([p], [g], [m], [v]), T.OptimTable([p], [g], [m])
    p0 = p.clone()

    def desc(**kw):
        d = _lib.OptimDesc()
        d.kind, d.has_v, d.lr_a, d.lr_b, d.momentum, d.eps = _lib.OPTIM_ADAMW, 1, 0.01, 0.0, 0.9, 1e-8
        d.beta1, d.beta2, d.bc1, d.sqrt_bc2, d.weight_decay, d.grad_scale = 0.9, 0.999, 0.1, math.sqrt(0.001), 0.01, 1.0
        d.clip, d.norm_type, d.partials, d.n_partials = _lib.CLIP_OFF, _lib.NORM_L2, part.data_ptr(), 1
        d.max_norm, d.clip_value, d.norm_out = 1.0, 1.0, part.data_ptr() + 4 * 256
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    def call(table, **kw):
        return lib.ledn_optim_step(table.table.data_ptr(), 1, 100, C.byref(desc(**kw)), None)
    nan = float('nan')
    bad = [dict(kind=2), dict(kind=-1), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan), dict(beta2=1.0), dict(beta2=-1e-3),
           dict(beta2=nan), dict(eps=0.0), dict(eps=-1e-8), dict(eps=nan), dict(has_v=0), dict(bc1=0.0), dict(sqrt_bc2=0.0),
           dict(clip=3), dict(clip=-1),
           dict(clip=_lib.CLIP_NORM, norm_type=_lib.NORM_NONE), dict(clip=_lib.CLIP_NORM, norm_type=1),
           dict(clip=_lib.CLIP_NORM, n_partials=0), dict(clip=_lib.CLIP_NORM, n_partials=257),
           dict(clip=_lib.CLIP_NORM, partials=None), dict(clip=_lib.CLIP_NORM, max_norm=0.0),
           dict(clip=_lib.CLIP_NORM, max_norm=-1.0), dict(clip=_lib.CLIP_NORM, max_norm=nan),
           dict(clip=_lib.CLIP_VALUE, clip_value=0.0), dict(clip=_lib.CLIP_VALUE, clip_value=-1.0),
           dict(clip=_lib.CLIP_VALUE, clip_value=nan)]
    for kw in bad:
        assert call(tab_v, **kw) == _lib.EINVAL, kw
    assert call(tab, kind=_lib.OPTIM_SGD, clip=7) == _lib.EINVAL
    assert lib.ledn_optim_step(None, 1, 100, C.byref(desc()), None) == _lib.EINVAL
    assert lib.ledn_optim_step(tab_v.table.data_ptr(), 0, 100, C.byref(desc()), None) == _lib.EINVAL
    assert lib.ledn_optim_step(tab_v.table.data_ptr(), 1, 0, C.byref(desc()), None) == _lib.EINVAL
    assert lib.ledn_optim_step(tab_v.table.data_ptr(), 1, 100, None, None) == _lib.EINVAL
    assert torch.equal(p, p0)                              # nothing was launched
    assert call(tab_v) == _lib.OK
    assert call(tab, kind=_lib.OPTIM_SGD, has_v=0) == _lib.OK          # SGD needs no second moments
    assert call(tab_v, clip=_lib.CLIP_NORM) == _lib.OK and call(tab_v, clip=_lib.CLIP_VALUE, partials=None) == _lib.OK
    assert C.sizeof(_lib.OptimEntry) == 48 and _lib.get_lib().cdll.ledn_abi_version() == 5
    with pytest.raises(_lib.LednError):
        T.OptimTable([p], [g], [m], [v], lr_mults=[1.0, 2.0])


# --------------------------------------------------------------------------- #
# 2. trajectory: 20 AdamW steps against torch in f32 and in f64
# --------------------------------------------------------------------------- #
def test_adamw_trajectory_error_vs_float64(be):
    """The kernel's distance from a float64 torch.optim.AdamW run may be at most 4x the distance of torch's own f32 run
    (a different but equally valid rounding order and FMA contraction).  Recorded in EXPERIMENTS.md."""
    from led_net_amd import _lib, ops_train as T
    sizes, steps = (20000, 4099, 7), 20
    g = torch.Generator().manual_seed(77)
    hp = [torch.randn(n, generator=g) for n in sizes]
    grads = [[torch.randn(n, generator=g) * (1.0 + 0.2 * math.sin(k)) for n in sizes] for k in range(steps)]
    lr, wd = 1e-3, 0.05
    runs = {}
    for dtype in (torch.float32, torch.float64):
        ref = [p.clone().to(dtype).requires_grad_(True) for p in hp]
        opt = torch.optim.AdamW(ref, lr=lr, betas=HYP['betas'], eps=HYP['eps'], weight_decay=wd)
        for k in range(steps):
            for r_, x in zip(ref, grads[k]):
                r_.grad = x.to(dtype)
            opt.step()
        runs[dtype] = [r_.detach().double() for r_ in ref]
    _, _, _, _, flat, pd, gd, md, vd = _table('AdamW', seed=0, sizes=sizes, p_off=(0, 1, 0))
    for p, x in zip(pd, hp):
        p.copy_(D(x))
    tab = T.OptimTable(pd, gd, md, vd)
    for k in range(steps):
        for gdev, x in zip(gd, grads[k]):
            gdev.copy_(D(x))
        tab.step(_lib.OPTIM_ADAMW, lr, 0.0, betas=HYP['betas'], eps=HYP['eps'], weight_decay=wd, t=k + 1)
    err_kernel = max(float((p.cpu().double() - w).abs().max()) for p, w in zip(pd, runs[torch.float64]))
    err_torch = max(float((a - w).abs().max()) for a, w in zip(runs[torch.float32], runs[torch.float64]))
    print(f'AdamW, {steps} steps: max |p - p_f64|: kernel {err_kernel:.3e}, torch f32 {err_torch:.3e}, '
          f'ratio {err_kernel / err_torch:.2f}')
    assert err_torch > 0 and err_kernel <= 4.0 * err_torch


# --------------------------------------------------------------------------- #
# 3. paramwise_cfg
# --------------------------------------------------------------------------- #
def _tiny_model():
    import led_net_amd as L
    return L.MODELS.build(L.load_config(CFG)['model']), L.load_config(CFG)


def _mults(model, cfg=None, **kw):
    import led_net_amd as L
    tr = L.Trainer(model, cfg, **kw)
    return dict(zip(tr.names, tr.mults)), tr


BN_W, BN_B = 'backbone.stem.0.bn.weight', 'backbone.stem.0.bn.bias'
DW = 'backbone.layer3_.0.spp_dw.0.conv.weight'
PRELU = 'backbone.layer3_.0.module_act.weight'
RPB = 'backbone.getb1.attn.relative_position_bias_table'
SEG_B, SEG_W = 'decode_head.conv_seg.bias', 'decode_head.conv_seg.weight'
FC_B = 'backbone.getb1.mlp.fc1.bias'
CONV = 'backbone.stem.0.conv.weight'


def test_paramwise_rules_by_parameter_name():
    model, cfg = _tiny_model()
    names = dict(model.named_parameters())
    assert all(k in names for k in (BN_W, BN_B, DW, PRELU, RPB, SEG_B, SEG_W, FC_B, CONV))
    assert names[DW].shape[1] == 1 and names[PRELU].ndim == 1 and names[RPB].ndim == 2
    m, tr = _mults(model, cfg)
    assert tr.paramwise is None and set(m.values()) == {(1.0, 1.0)} and not tr._general
    m, tr = _mults(model, cfg, paramwise_cfg=dict(norm_decay_mult=0.))
    assert tr._general
    assert m[BN_W] == (1.0, 0.0) and m[BN_B] == (1.0, 0.0)
    assert m[CONV] == m[SEG_B] == m[PRELU] == m[RPB] == m[DW] == (1.0, 1.0)
    # a custom key wins over every other rule, for the parameters it matches
    m, _ = _mults(model, cfg, paramwise_cfg=dict(custom_keys={'decode_head': dict(lr_mult=10.)}, bias_decay_mult=0.,
                                                 bias_lr_mult=2.))
    assert m[SEG_B] == (10.0, 1.0) and m[SEG_W] == (10.0, 1.0)
    assert m[FC_B] == (2.0, 0.0)                      # a convolution's bias outside the custom key
    assert m[BN_B] == (1.0, 0.0)                      # a norm layer's bias: bias_decay_mult yes, bias_lr_mult no
    assert m[BN_W] == (1.0, 1.0)
    m, _ = _mults(model, cfg, paramwise_cfg=dict(norm_decay_mult=0.5, bias_decay_mult=0.25))
    assert m[BN_B] == (1.0, 0.5) and m[FC_B] == (1.0, 0.25)          # the norm rule comes first
    m, _ = _mults(model, cfg, paramwise_cfg=dict(dwconv_decay_mult=0.1, flat_decay_mult=0.3))
    assert m[DW] == (1.0, 0.1) and m[CONV] == (1.0, 1.0)
    assert m[PRELU] == (1.0, 0.3) and m[BN_W] == (1.0, 0.3) and m[FC_B] == (1.0, 0.3)     # every 1-d parameter
    assert m[RPB] == (1.0, 1.0)                       # 2-d, its module is no norm layer, no bias: nothing applies
    m, _ = _mults(model, cfg, paramwise_cfg=dict(norm_decay_mult=0., bias_decay_mult=0., dwconv_decay_mult=0.,
                                                 flat_decay_mult=0., bias_lr_mult=3.))
    assert m[RPB] == (1.0, 1.0) and m[CONV] == (1.0, 1.0) and m[PRELU] == (1.0, 0.0)
    # the config's optim_wrapper section is read when the argument is absent; bypass_duplicate is accepted
    cfg['optim_wrapper'] = dict(type='OptimWrapper', optimizer=cfg['optimizer'],
                                paramwise_cfg=dict(norm_decay_mult=0., bypass_duplicate=True))
    m, tr = _mults(model, cfg)
    assert m[BN_W] == (1.0, 0.0) and (tr.base_lr, tr.momentum, tr.wd) == (0.01, 0.9, 5e-4)


def test_paramwise_custom_keys_longest_first_then_alphabetical():
    model, cfg = _tiny_model()
    m, _ = _mults(model, cfg, paramwise_cfg=dict(custom_keys={
        'backbone': dict(lr_mult=0.1), 'backbone.stem': dict(lr_mult=0.5, decay_mult=0.), 'decode_head': dict(lr_mult=10.)}))
    assert m[CONV] == (0.5, 0.0) and m[BN_W] == (0.5, 0.0)            # the longer key, although 'backbone' matches too
    assert m[DW] == (0.1, 1.0) and m[SEG_B] == (10.0, 1.0)
    # equal lengths: alphabetical order decides ('.stem.' < 'stem.0')
    m, _ = _mults(model, cfg, paramwise_cfg=dict(custom_keys={'stem.0': dict(lr_mult=7.), '.stem.': dict(lr_mult=3.)}))
    assert m[CONV] == (3.0, 1.0) and m['backbone.stem.1.conv.weight'] == (3.0, 1.0) and m[DW] == (1.0, 1.0)


@pytest.mark.parametrize('bad,word', [
    (dict(dcn_offset_lr_mult=0.1), 'dcn_offset_lr_mult'), (dict(norm_decay_mlt=0.), 'norm_decay_mlt'),
    (dict(custom_keys={'head': dict(lr_mul=2.)}), 'lr_mul'), (dict(custom_keys=['head']), 'custom_keys'),
    (dict(custom_keys={'head': 2.0}), 'custom_keys'), ([('norm_decay_mult', 0.)], 'dict')])
def test_bad_paramwise_cfg_raises_value_error(bad, word):
    import led_net_amd as L
    model, cfg = _tiny_model()
    with pytest.raises(ValueError, match=word):
        L.Trainer(model, cfg, paramwise_cfg=bad)
    cfg['optim_wrapper'] = dict(paramwise_cfg=bad)
    with pytest.raises(ValueError, match=word):
        L.Trainer(model, cfg)


# --------------------------------------------------------------------------- #
# 4. schedules
# --------------------------------------------------------------------------- #
def _torch_lrs(cls, base, steps, **kw):
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([p], lr=base)
    sch = cls(opt, **kw)
    out = [sch.get_last_lr()[0]]
    for _ in range(steps):
        opt.step()
        sch.step()
        out.append(sch.get_last_lr()[0])
    return out


def test_warmup_then_poly_schedule_vs_torch_and_closed_form():
    import led_net_amd as L
    from torch.optim.lr_scheduler import LinearLR, PolynomialLR
    model, cfg = _tiny_model()
    base, w, end = 6e-5, 1500, 20000
    cfg['optimizer'] = dict(type='SGD', lr=base, momentum=0.9, weight_decay=0.01)
    cfg['param_scheduler'] = [dict(type='LinearLR', start_factor=1e-6, by_epoch=False, begin=0, end=w),
                              dict(type='PolyLR', eta_min=0.0, power=0.9, begin=w, end=end, by_epoch=False)]
    tr = L.Trainer(model, cfg)
    assert tr.max_iters == end and tr._general
    lin = _torch_lrs(LinearLR, base, w, start_factor=1e-6, end_factor=1.0, total_iters=w)
    poly = _torch_lrs(PolynomialLR, base, end - w, total_iters=end - w, power=0.9)

    def at(t):
        tr.iter = t
        return tr.lr()
    # torch's schedulers run the recursive ("chainable") form in double: ~1e-16 per step over <= 2e4 steps
    for t in (0, 1, 2, 750, w - 1):
        assert at(t) == pytest.approx(lin[t], rel=1e-9), t
        assert at(t) == pytest.approx(base * (1e-6 + (1 - 1e-6) * t / w), rel=1e-14)
    assert at(0) == pytest.approx(base * 1e-6, rel=1e-12) and at(w) == pytest.approx(base, rel=1e-12)
    for t in (w, w + 1, 5000, 12345, end - 1, end, end + 10):
        assert at(t) == pytest.approx(poly[min(t, end) - w], rel=1e-9, abs=1e-20), t
    assert at(end) == 0.0 and at(end + 10) == 0.0 and at(w - 1) < at(w) > at(w + 1)
    # eta_min != 0 (torch's PolynomialLR has none): the written closed form; a gap between the intervals holds the value
    cfg['param_scheduler'] = [dict(type='LinearLR', start_factor=0.1, end_factor=0.5, by_epoch=False, begin=0, end=100),
                              dict(type='PolyLR', eta_min=1e-6, power=2.0, begin=150, end=1150, by_epoch=False)]
    tr = L.Trainer(model, cfg, paramwise_cfg=dict(custom_keys={'decode_head': dict(lr_mult=10.)}))
    for t, want in ((0, base * 0.1), (50, base * 0.3), (100, base * 0.5), (120, base * 0.5), (149, base * 0.5),
                    (150, base * 0.5), (650, (base * 0.5 - 1e-6) * 0.25 + 1e-6), (1150, 1e-6), (5000, 1e-6)):
        tr.iter = t
        assert tr.lr() == pytest.approx(want, rel=1e-12), t
        # a group with lr_mult 10 follows ITS closed form (base rate 10 * base), through the two scalars of the kernel
        a, b = tr.sched.scalars(tr.base_lr, t)
        f = (1.0 - (min(max(t, 150), 1150) - 150) / 1000) ** 2.0
        want10 = (10 * base * 0.1 * (1 + 4 * min(t, 100) / 100)) if t < 150 else (10 * base * 0.5 - 1e-6) * f + 1e-6
        assert 10.0 * a + b == pytest.approx(want10, rel=1e-12), t
        assert 1.0 * a + b == pytest.approx(tr.lr(), rel=1e-12), t
    # ConstantLR: factor inside [begin, end), the base rate again from `end` on (torch's ConstantLR)
    from torch.optim.lr_scheduler import ConstantLR
    cfg['param_scheduler'] = [dict(type='ConstantLR', factor=0.25, by_epoch=False, begin=0, end=30)]
    tr = L.Trainer(model, cfg)
    con = _torch_lrs(ConstantLR, base, 40, factor=0.25, total_iters=30)
    for t in (0, 29, 30, 40):
        tr.iter = t
        assert tr.lr() == pytest.approx(con[t], rel=1e-12), t


def test_single_polylr_values_are_the_parent_commits_bits():
    """Trainer.lr() under the existing single-PolyLR configs: values recorded from the commit before this change"""
    import led_net_amd as L
    model, cfg = _tiny_model()
    tr = L.Trainer(model, cfg, max_iters=1000)
    assert not tr._general
    for it, want in ((0, 0.01), (1, 0.009990999549834914), (500, 0.005358867312681466), (999, 1.995262314968881e-05),
                     (1000, 0.0), (1500, 0.0)):
        tr.iter = it
        assert tr.lr() == want, it
    cfg['param_scheduler'][0]['eta_min'] = 1e-4
    tr = L.Trainer(model, cfg)
    tr.iter = 12345
    assert tr.max_iters == 80000 and tr.lr() == 0.008613813154420431
    tr = L.Trainer(model, None, lr=6e-5, max_iters=160000)           # no config: PolyLR(power=0.9, eta_min=0) over max_iters
    tr.iter = 777
    assert tr.lr() == 5.9737698711786604e-05
    sd = tr.scheduler_state_dict()
    assert sd['last_step'] == 777 and sd['end'] == 160000 and sd['base_values'] == [6e-5]


# --------------------------------------------------------------------------- #
# 5. configuration errors
# --------------------------------------------------------------------------- #
def _lin(b, e, **kw):
    return dict(type='LinearLR', by_epoch=False, begin=b, end=e, **kw)


def _poly(b, e, **kw):
    return dict(type='PolyLR', by_epoch=False, begin=b, end=e, **kw)


@pytest.mark.parametrize('opt,word', [
    (dict(type='Adam', lr=1e-3), 'Adam'), (dict(type='Lion', lr=1e-3), 'Lion'),
    (dict(type='AdamW', lr=1e-3, amsgrad=True), 'amsgrad'), (dict(type='SGD', lr=0.01, nesterov=True), 'nesterov'),
    (dict(type='SGD', lr=0.01, dampening=0.1), 'dampening'), (dict(type='AdamW', lr=1e-3, betas=(0.9, 1.0)), 'betas'),
    (dict(type='AdamW', lr=1e-3, eps=0.0), 'eps'), (dict(type='AdamW', lr=1e-3, momentum=0.9), 'momentum'),
    (dict(type='SGD', lr=0.01, beta=(0.9, 0.99)), 'beta')])
def test_bad_optimizer_raises_value_error(opt, word):
    import led_net_amd as L
    model, cfg = _tiny_model()
    cfg['optimizer'] = opt
    with pytest.raises(ValueError, match=word):
        L.Trainer(model, cfg)
    cfg = L.load_config(CFG)
    cfg['optim_wrapper'] = dict(type='OptimWrapper', optimizer=opt)           # wins over cfg['optimizer']
    with pytest.raises(ValueError, match=word):
        L.Trainer(model, cfg)


@pytest.mark.parametrize('sched,word', [
    ([_lin(0, 1500), _poly(1000, 2000)], 'overlap'), ([_poly(0, 2000), _lin(0, 1500)], 'overlap'),
    ([dict(type='LinearLR', by_epoch=True, begin=0, end=5), _poly(5, 100)], 'by_epoch'),
    ([dict(type='PolyLR', by_epoch=True, begin=0, end=100)], 'by_epoch'),
    ([dict(type='LinearLR', begin=0, end=5), _poly(5, 100)], 'by_epoch'),       # mmengine's default is by_epoch=True
    ([dict(type='CosineAnnealingLR', by_epoch=False, begin=0, end=100)], 'CosineAnnealingLR'),
    ([_lin(0, 10), dict(type='OneCycleLR', by_epoch=False, begin=10, end=100)], 'OneCycleLR'),
    ([_lin(0, 10, start_factr=0.1)], 'start_factr'), ([_lin(10, 10)], 'begin'), ([_lin(0, 10), dict(type='PolyLR', by_epoch=False, begin=10)], 'end')])
def test_bad_param_scheduler_raises_value_error(sched, word):
    import led_net_amd as L
    model, cfg = _tiny_model()
    cfg['param_scheduler'] = sched
    with pytest.raises(ValueError, match=word):
        L.Trainer(model, cfg)


def test_adamw_is_read_from_the_config_and_arguments_win():
    import led_net_amd as L
    model, cfg = _tiny_model()
    cfg['optim_wrapper'] = dict(type='OptimWrapper', optimizer=dict(type='AdamW', lr=6e-5, betas=(0.8, 0.99), weight_decay=0.02))
    tr = L.Trainer(model, cfg)
    assert (tr.opt_kind, tr.base_lr, tr.betas, tr.eps, tr.wd) == ('AdamW', 6e-5, (0.8, 0.99), 1e-8, 0.02)
    assert tr._general and tr.flat_v is not None and tr.flat_v.shape == tr.flat_mom.shape
    tr = L.Trainer(model, cfg, lr=1e-4, weight_decay=0.0)
    assert (tr.base_lr, tr.wd) == (1e-4, 0.0)
    cfg['optim_wrapper']['optimizer'] = dict(type='AdamW')
    tr = L.Trainer(model, cfg)
    assert (tr.betas, tr.eps, tr.wd) == ((0.9, 0.999), 1e-8, 1e-2)
    del cfg['optim_wrapper']
    tr = L.Trainer(model, cfg)                        # the config's own SGD: no second moments
    assert tr.opt_kind == 'SGD' and tr.flat_v is None and not tr._general
    cfg['param_scheduler'] = [_lin(0, 10), _poly(10, 500, power=0.9)]
    tr = L.Trainer(model, cfg)
    assert tr._general and tr.max_iters == 500 and len(tr.scheduler_state_dicts()) == 2


# --------------------------------------------------------------------------- #
# 6. the whole step: AdamW + paramwise_cfg + warm-up + norm clipping
# --------------------------------------------------------------------------- #
PARAMWISE = dict(norm_decay_mult=0., bias_decay_mult=0., custom_keys={'decode_head': dict(lr_mult=10.)})


def _adamw_cfg(cfg):
    cfg = copy.deepcopy(cfg)
    for c in cfg['model']['decode_head']['loss_decode']:
        c['min_kept'] = 20000
    cfg['optim_wrapper'] = dict(type='OptimWrapper', optimizer=dict(type='AdamW', lr=1e-3, betas=(0.9, 0.999), weight_decay=0.05),
                                paramwise_cfg=copy.deepcopy(PARAMWISE))
    cfg['param_scheduler'] = [dict(type='LinearLR', start_factor=0.1, by_epoch=False, begin=0, end=5),
                              dict(type='PolyLR', eta_min=1e-6, power=0.9, begin=5, end=50, by_epoch=False)]
    return cfg


def _batch(dev, seed=11, batch=2):
    import led_net_amd as L
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (batch, 3, 320, 320), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 2, (batch, 1, 320, 320), dtype=torch.int64, generator=g)
    lab[:, :, :6, :] = 255
    return img, [L.SegDataSample(gt=lab[i].to(dev)) for i in range(batch)]


def _adamw_trainer(dev, seed=304, **kw):
    import led_net_amd as L
    torch.manual_seed(seed)
    cfg = _adamw_cfg(L.load_config(CFG))
    model = L.MODELS.build(cfg['model']).to(dev)
    return L.Trainer(model, cfg, **kw), model, cfg


def _whole_step_case(dev):
    tr, model, cfg = _adamw_trainer(dev)
    img, samples = _batch(dev)
    assert tr.opt_kind == 'AdamW' and tr._general and tr.max_iters == 50
    out = tr.train_step(img, samples)                       # no clipping yet: attaches the flat gradient views / sinks
    assert 'grad_norm' not in out and tr._sink_map and tr.iter == 1
    assert float(tr.flat_v.abs().max()) > 0 and float(tr.flat_grad.abs().max()) == 0.0
    state = {k: v.clone() for k, v in model.state_dict().items()}
    tr.forward_backward(img, samples)
    live = [i for i, p in enumerate(tr.params) if any(p is q for q in tr.live)]
    grads = [tr.views[i].detach().cpu().clone() for i in live]
    flat = tr.flat_grad.detach().cpu().clone()
    model.load_state_dict(state)                            # the running statistics moved in that forward
    params = [tr.params[i].detach().cpu().clone() for i in live]
    ms = [tr.moms[i].detach().cpu().clone() for i in live]
    vs = [tr.vs[i].detach().cpu().clone() for i in live]
    measured = float(torch.linalg.vector_norm(flat.double(), 2.0))
    assert math.isfinite(measured) and measured > 0
    tr.flat_grad.zero_()
    tr.set_clip_grad(dict(max_norm=0.5 * measured))
    # the rates of step 2 (iter 1 of the warm-up): base * (0.1 + 0.9 * 1/5), ten times that in the decode head
    assert tr.lr() == pytest.approx(1e-3 * (0.1 + 0.9 / 5), rel=1e-12)
    a, b = tr.sched.scalars(tr.base_lr, tr.iter)
    out = tr.train_step(img, samples)
    ref = [p.double().requires_grad_(True) for p in params]
    groups, seen = [], set()
    for r_, i in zip(ref, live):
        lm, dm = tr.mults[i]
        seen.add((lm, dm))
        groups.append(dict(params=[r_], lr=lm * a + b, weight_decay=dm * tr.wd))
    assert {(1.0, 1.0), (1.0, 0.0), (10.0, 1.0)} <= seen
    opt = torch.optim.AdamW(groups, betas=tr.betas, eps=tr.eps)
    for r_, g_, m_, v_ in zip(ref, grads, ms, vs):
        r_.grad = g_.double()
        opt.state[r_] = {'step': torch.tensor(1.0), 'exp_avg': m_.double(), 'exp_avg_sq': v_.double()}
    want_norm = torch.nn.utils.clip_grad_norm_(ref, 0.5 * measured)
    used = [r_.grad.clone() for r_ in ref]
    opt.step()
    coef, got_norm = float(tr.clip.coef), out['grad_norm'].cpu()
    print(f'AdamW whole step: grad_norm {float(got_norm):.6g} (torch {float(want_norm):.6g}), coef {coef:.6g}')
    assert coef < 1.0
    torch.testing.assert_close(got_norm, want_norm.float(), rtol=RTOL, atol=0)
    assert tuple(tr.betas) == HYP['betas'] and tr.eps == HYP['eps']
    for i, r_, p0, m0, g_, grp in zip(live, ref, params, ms, used, groups):
        got = tr.params[i].detach().cpu()
        scale = _update_scale('AdamW', p0, m0, g_, grp['lr'], grp['weight_decay'], opt.state[r_]['exp_avg_sq'], 2)
        _assert_within(got.double() - p0.double(), r_.detach().double() - p0.double(), scale, f'update {tr.names[i]}', k=2.0)
        _assert_within(tr.moms[i], opt.state[r_]['exp_avg'], m0.abs() + g_.abs(), f'exp_avg {tr.names[i]}')
        torch.testing.assert_close(tr.vs[i].detach().cpu().double(), opt.state[r_]['exp_avg_sq'], rtol=RTOL, atol=1e-30)
    assert float(tr.flat_grad.abs().max()) == 0.0 and tr.iter == 2


def test_adamw_whole_step_vs_torch(emu):
    _whole_step_case(torch.device('cpu'))


@pytest.mark.gpu
def test_adamw_whole_step_vs_torch_gpu():
    import led_net_amd as L
    L.set_deterministic(True)           # the gradients of the two passes are then the same bits
    try:
        _whole_step_case(torch.device('cuda:0'))
    finally:
        L.set_deterministic(False)


def _warm(tr, model, batch):
    """two real steps, then everything put back (what capture(restore=True) does): the steps that follow all run the
    steady-state path of the trainer, whatever came before"""
    snap = ([p.detach().clone() for p in tr.params], [b_.detach().clone() for b_ in model.buffers()], tr.iter,
            tr.flat_mom.clone(), tr.flat_v.clone())
    for _ in range(2):
        tr.train_step(*batch)
    with torch.no_grad():
        for p, v in zip(tr.params, snap[0]):
            p.copy_(v)
        for b_, v in zip(model.buffers(), snap[1]):
            b_.copy_(v)
        tr.flat_mom.copy_(snap[3])
        tr.flat_v.copy_(snap[4])
    tr.iter = snap[2]


def _run_steps(dev, batches, init, tmp_path=None, mode='eager', clip=dict(max_norm=0.05)):
    """mode: 'eager', 'graph' (capture + replay) or 'resume' (two steps, checkpoint, a NEW trainer continues)"""
    import led_net_amd as L
    tr, model, cfg = _adamw_trainer(dev, clip_grad=clip)
    model.load_state_dict(init)
    outs, ck = [], None
    if mode == 'graph':
        tr.capture(*batches[0], warmup=2, restore=True)
        assert tr.iter == 0 and float(tr.flat_v.abs().max()) == 0.0 and tr._lr_dev.numel() == 4
        for b in batches:
            o = tr.replay(*b)
            outs.append({k: v.detach().clone() for k, v in o.items()})
    else:
        _warm(tr, model, batches[0])
        for k, b in enumerate(batches):
            if mode == 'resume' and k == 2:
                path = str(tmp_path / 'iter_2.pth')
                L.save_checkpoint(model, path, meta=dict(iter=2), trainer=tr)
                tr, model, cfg = _adamw_trainer(dev, seed=999, clip_grad=clip)
                ck = L.load_checkpoint(model, path)
                L.resume(tr, ck)
                assert tr.iter == 2
                _warm(tr, model, batches[0])
            o = tr.train_step(*b)
            outs.append({k_: v.detach().clone() for k_, v in o.items()})
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return outs, {k: v.detach().clone() for k, v in model.state_dict().items()}, tr.flat_mom.clone(), tr.flat_v.clone(), tr, ck


def _same(a, b):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        for k in x:
            assert torch.equal(x[k], y[k]), (i, k, x[k], y[k])
    bad = [k for k in a[1] if not torch.equal(a[1][k], b[1][k])]
    assert not bad, bad[:5]
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def _check_adamw_checkpoint(ck, model, tr):
    """the saved 'optimizer' is torch.optim.AdamW's own layout: torch loads it over per-parameter groups"""
    opt_sd, n = ck['optimizer'], len(list(model.parameters()))
    assert len(opt_sd['param_groups']) == n and [g['params'] for g in opt_sd['param_groups']] == [[i] for i in range(n)]
    assert 0 < len(opt_sd['state']) < n
    idx = {name: i for i, (name, _) in enumerate(model.named_parameters())}
    g_bn, g_head, g_conv = (opt_sd['param_groups'][idx[k]] for k in (BN_W, SEG_B, CONV))
    assert g_bn['weight_decay'] == 0.0 and g_conv['weight_decay'] == 0.05 and g_head['initial_lr'] == pytest.approx(1e-2)
    assert g_head['lr'] == pytest.approx(10 * g_conv['lr'], rel=1e-3) and g_conv['betas'] == (0.9, 0.999)
    assert g_conv['amsgrad'] is False and g_conv['eps'] == 1e-8
    assert len(ck['param_schedulers']) == 2 and all(s['last_step'] == 2 for s in ck['param_schedulers'])
    assert len(ck['param_schedulers'][0]['base_values']) == n
    ref = [p.detach().cpu().clone().requires_grad_(True) for p in model.parameters()]
    topt = torch.optim.AdamW([dict(params=[r_]) for r_ in ref], lr=1e-3)
    topt.load_state_dict(opt_sd)
    k = next(iter(opt_sd['state']))
    st = topt.state[ref[k]]
    assert float(st['step']) == 2.0 and st['step'].dtype == torch.float32
    assert torch.equal(st['exp_avg'], opt_sd['state'][k]['exp_avg']) and torch.equal(st['exp_avg_sq'], opt_sd['state'][k]['exp_avg_sq'])
    assert topt.param_groups[idx[BN_W]]['weight_decay'] == 0.0


def _determinism_case(dev, tmp_path, graph):
    import led_net_amd as L
    L.set_deterministic(True)
    try:
        batches = [_batch(dev, seed=23 + k) for k in range(4)]
        _, model, _ = _adamw_trainer(dev)
        init = copy.deepcopy(model.state_dict())
        eager = _run_steps(dev, batches, init)
        assert float(eager[4].clip.coef) < 1.0 and eager[4].iter == 4
        _same(eager, _run_steps(dev, batches, init))                             # two runs
        resumed = _run_steps(dev, batches, init, tmp_path, mode='resume')
        _same((eager[0][2:],) + eager[1:], (resumed[0][2:],) + resumed[1:])      # resumed = uninterrupted
        _check_adamw_checkpoint(resumed[5], resumed[4].model, resumed[4])
        if graph:
            _same(eager, _run_steps(dev, batches, init, mode='graph'))           # capture + replay = eager
        # the other optimizer's checkpoint is refused
        cfg = L.load_config(CFG)
        sgd = L.Trainer(L.MODELS.build(cfg['model']).to(dev), cfg)
        with pytest.raises(ValueError, match='AdamW'):
            sgd.load_optimizer_state_dict(resumed[5]['optimizer'])
        with pytest.raises(ValueError, match='SGD'):
            eager[4].load_optimizer_state_dict({'state': {0: {'momentum_buffer': torch.zeros(1)}},
                                                'param_groups': [dict(momentum=0.9, params=[0])]})
    finally:
        L.set_deterministic(False)


def test_adamw_two_runs_and_resume_are_bit_identical(emu, tmp_path):
    slow_on_emu(torch.device('cpu'))
    _determinism_case(torch.device('cpu'), tmp_path, graph=False)


@pytest.mark.gpu
def test_adamw_two_runs_replay_and_resume_are_bit_identical_gpu(tmp_path):
    _determinism_case(torch.device('cuda:0'), tmp_path, graph=True)


def test_adamw_checkpoint_layout_and_optimizer_mismatch(emu, tmp_path):
    """(the CPU suite's share of the resume test: two steps, the checkpoint, torch.optim.AdamW loads it, the restored
    trainer holds the same moments, step and rates)"""
    import led_net_amd as L
    dev = torch.device('cpu')
    tr, model, cfg = _adamw_trainer(dev)
    b = _batch(dev, batch=1)
    tr.train_step(*b)
    tr.train_step(*b)
    path = str(tmp_path / 'iter_2.pth')
    L.save_checkpoint(model, path, meta=dict(iter=2), trainer=tr)
    tb, mb, _ = _adamw_trainer(dev, seed=1)
    ck = L.load_checkpoint(mb, path)
    _check_adamw_checkpoint(ck, mb, tb)
    tb.iter = 0
    tb.load_optimizer_state_dict(ck['optimizer'])           # without schedulers: AdamW's step count sets the iteration
    assert tb.iter == 2
    L.resume(tb, ck)
    assert tb.iter == 2 and tb.lr() == tr.lr() and tb._optim_scalars() == tr._optim_scalars()
    pa, pb = {id(p): i for i, p in enumerate(tr.params)}, {id(p): i for i, p in enumerate(tb.params)}
    for p_a, p_b in zip(model.parameters(), mb.parameters()):
        assert torch.equal(tr.moms[pa[id(p_a)]], tb.moms[pb[id(p_b)]]) and torch.equal(tr.vs[pa[id(p_a)]], tb.vs[pb[id(p_b)]])
    assert float(tb.flat_v.abs().max()) > 0
    sgd = L.Trainer(L.MODELS.build(L.load_config(CFG)['model']), L.load_config(CFG))
    with pytest.raises(ValueError, match='AdamW'):
        sgd.load_optimizer_state_dict(ck['optimizer'])
    with pytest.raises(ValueError, match='SGD'):
        tb.load_optimizer_state_dict({'state': {0: {'momentum_buffer': torch.zeros(1)}},
                                      'param_groups': [dict(momentum=0.9, params=[0])]})


# --------------------------------------------------------------------------- #
# 7. the command line
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
def test_train_cli_takes_adamw_from_cfg_options(tmp_path):
    def run(extra, wd):
        env = dict(os.environ, PYTHONPATH=ROOT, LEDN_DETERMINISTIC='1')
        args = [sys.executable, 'tools/train.py', CFG, '--max-iters', '3', '--batch-size', '2', '--height', '320',
                '--width', '320', '--f32', '--work-dir', str(tmp_path / wd)] + extra
        r = subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, f'{args}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
        line = [ln for ln in r.stdout.splitlines() if re.search(r'\[\s*3/3\]', ln)]
        assert line, r.stdout[-2000:]
        return line[0]
    plain = run([], 'plain')
    adamw = run(['--cfg-options', 'optim_wrapper.optimizer.type=AdamW', 'optim_wrapper.optimizer.lr=0.001'], 'adamw')
    pw = run(['--cfg-options', 'optim_wrapper.optimizer.type=AdamW', 'optim_wrapper.optimizer.lr=0.001',
              'optim_wrapper.paramwise_cfg.norm_decay_mult=0.', "optim_wrapper.paramwise_cfg.custom_keys={'decode_head': {'lr_mult': 10.}}"],
             'paramwise')
    print(plain, adamw, pw, sep='\n')
    loss = [re.search(r'loss_context: ([0-9.eE+-]+)', ln).group(1) for ln in (plain, adamw, pw)]
    assert all(math.isfinite(float(x)) for x in loss)
    assert len(set(loss)) == 3                  # AdamW changes the run, and so does the paramwise_cfg on top of it
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, 'tools/train.py', CFG, '--max-iters', '1', '--work-dir', str(tmp_path / 'bad'),
                        '--cfg-options', 'optim_wrapper.optimizer.type=Adam'], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode != 0 and 'ValueError' in r.stderr and 'Adam' in r.stderr
