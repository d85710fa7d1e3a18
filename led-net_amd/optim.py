"""Optimizer construction from the config: what mmengine's build_optim_wrapper / DefaultOptimWrapperConstructor /
param_scheduler list do for the keys this project honours, restated here (mmengine is not a dependency; DESIGN.md
"Optimizer construction from the config" is the contract).  Everything in this file is host-side and runs once; the
per-step work is ONE launch (ops_train.OptimTable.step, or SgdTable.step for a plain SGD configuration).

A key is either honoured or rejected with ValueError -- nothing in the optimizer section is silently ignored."""
import math

import torch.nn as nn

_NORMS = (nn.modules.batchnorm._BatchNorm, nn.GroupNorm, nn.LayerNorm, nn.modules.instancenorm._InstanceNorm)


# --------------------------------------------------------------------------- #
# optimizer = dict(type='SGD' | 'AdamW', ...)
# --------------------------------------------------------------------------- #
_SGD_KEYS = {'type', 'lr', 'momentum', 'weight_decay', 'dampening', 'nesterov', 'maximize', 'foreach', 'differentiable',
             'fused'}
_ADAMW_KEYS = {'type', 'lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'maximize', 'foreach', 'capturable',
               'differentiable', 'fused'}


def parse_optimizer(opt, lr=None, momentum=None, weight_decay=None):
    """the config's optimizer dict (+ the Trainer's constructor arguments, which win) ->
    dict(kind='SGD', lr, momentum, weight_decay) or dict(kind='AdamW', lr, betas, eps, weight_decay)"""
    opt = dict(opt or {})
    kind = opt.get('type', 'SGD')
    if kind not in ('SGD', 'AdamW'):
        raise ValueError(f"optimizer: type={kind!r} is not supported (supported: 'SGD', 'AdamW')")
    unknown = sorted(set(opt) - (_SGD_KEYS if kind == 'SGD' else _ADAMW_KEYS))
    if unknown:
        raise ValueError(f'optimizer (type={kind!r}): unknown key {unknown[0]!r}')
    if opt.get('maximize', False):
        raise ValueError('optimizer: maximize=True is not supported')
    if kind == 'SGD':
        if opt.get('nesterov', False):
            raise ValueError('optimizer: nesterov=True is not supported')
        if opt.get('dampening', 0) != 0:
            raise ValueError(f'optimizer: dampening={opt["dampening"]!r} is not supported (only 0)')
        return dict(kind='SGD', lr=lr if lr is not None else opt.get('lr', 0.01),
                    momentum=momentum if momentum is not None else opt.get('momentum', 0.9),
                    weight_decay=weight_decay if weight_decay is not None else opt.get('weight_decay', 5e-4))
    if opt.get('amsgrad', False):
        raise ValueError('optimizer: amsgrad=True is not supported')
    if momentum is not None:
        raise ValueError("optimizer: momentum= does not apply to type='AdamW' (use betas)")
    betas = tuple(float(b) for b in opt.get('betas', (0.9, 0.999)))
    eps = float(opt.get('eps', 1e-8))
    if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
        raise ValueError(f'optimizer: betas={opt.get("betas")!r} must be two values in [0, 1)')
    if not eps > 0:
        raise ValueError(f'optimizer: eps={opt.get("eps")!r} must be > 0')
    return dict(kind='AdamW', lr=lr if lr is not None else opt.get('lr', 1e-3), betas=betas, eps=eps,
                weight_decay=weight_decay if weight_decay is not None else opt.get('weight_decay', 1e-2))


# --------------------------------------------------------------------------- #
# optim_wrapper.paramwise_cfg
# --------------------------------------------------------------------------- #
_PARAMWISE_KEYS = {'custom_keys', 'bias_lr_mult', 'bias_decay_mult', 'norm_decay_mult', 'dwconv_decay_mult',
                   'flat_decay_mult', 'bypass_duplicate'}


def parse_paramwise(pw):
    """validate paramwise_cfg -> None (nothing to do) or a normalised dict; unknown keys and dcn_offset_lr_mult raise"""
    if pw is None:
        return None
    if not isinstance(pw, dict):
        raise ValueError(f'paramwise_cfg must be None or a dict, got {type(pw).__name__}')
    if 'dcn_offset_lr_mult' in pw:
        raise ValueError('paramwise_cfg: dcn_offset_lr_mult is not supported (the model has no deformable convolution)')
    unknown = sorted(set(pw) - _PARAMWISE_KEYS)
    if unknown:
        raise ValueError(f'paramwise_cfg: unknown key {unknown[0]!r}')
    out = {}
    for k in _PARAMWISE_KEYS - {'custom_keys', 'bypass_duplicate'}:
        if pw.get(k) is not None:
            out[k] = float(pw[k])
    ck = pw.get('custom_keys') or {}
    if not isinstance(ck, dict):
        raise ValueError('paramwise_cfg: custom_keys must be a dict')
    custom = {}
    for key, val in ck.items():
        if not isinstance(key, str) or not isinstance(val, dict):
            raise ValueError(f'paramwise_cfg: custom_keys[{key!r}] must map a name to a dict')
        bad = sorted(set(val) - {'lr_mult', 'decay_mult'})
        if bad:
            raise ValueError(f'paramwise_cfg: custom_keys[{key!r}]: unknown key {bad[0]!r}')
        custom[key] = (float(val.get('lr_mult', 1.0)), float(val.get('decay_mult', 1.0)))
    if custom:
        out['custom_keys'] = custom
    return out or None


def paramwise_multipliers(model, pw):
    """-> {parameter name: (lr_mult, decay_mult)} for every parameter with requires_grad, by the rules of mmengine's
    DefaultOptimWrapperConstructor.add_params (pw: the result of parse_paramwise)"""
    pw = pw or {}
    custom = pw.get('custom_keys', {})
    keys = sorted(sorted(custom), key=len, reverse=True)        # by length, longest first; equal lengths alphabetically
    out = {}
    for mod_name, mod in model.named_modules():
        is_norm = isinstance(mod, _NORMS)
        is_dw = isinstance(mod, nn.Conv2d) and mod.in_channels == mod.groups
        for pname, p in mod.named_parameters(recurse=False):
            full = f'{mod_name}.{pname}' if mod_name else pname
            if not p.requires_grad or full in out:
                continue
            hit = next((k for k in keys if k in full), None)
            if hit is not None:                                 # a custom key: its two multipliers and nothing else
                out[full] = custom[hit]
                continue
            lr_mult, decay_mult = 1.0, 1.0
            if pname == 'bias' and not is_norm and 'bias_lr_mult' in pw:
                lr_mult = pw['bias_lr_mult']
            if is_norm and 'norm_decay_mult' in pw:
                decay_mult = pw['norm_decay_mult']
            elif pname == 'bias' and 'bias_decay_mult' in pw:
                decay_mult = pw['bias_decay_mult']
            elif is_dw and 'dwconv_decay_mult' in pw:
                decay_mult = pw['dwconv_decay_mult']
            elif p.ndim == 1 and 'flat_decay_mult' in pw:
                decay_mult = pw['flat_decay_mult']
            out[full] = (lr_mult, decay_mult)
    return out


# --------------------------------------------------------------------------- #
# param_scheduler = [dict(type='LinearLR' | 'PolyLR' | 'ConstantLR', by_epoch=False, begin=, end=, ...), ...]
# --------------------------------------------------------------------------- #
_SCHED_KEYS = {'LinearLR': {'start_factor', 'end_factor'}, 'PolyLR': {'power', 'eta_min'}, 'ConstantLR': {'factor'}}
_SCHED_COMMON = {'type', 'by_epoch', 'begin', 'end', 'last_step', 'verbose'}


class Schedule:
    """The config's scheduler list by iteration.  A group of base rate lr_mult * base_lr has, at step t, the rate
    lr_mult * A(t) + B(t) (scalars()); value() is that rate for the base group (lr_mult = 1) by the closed forms
    themselves, so a lone PolyLR returns the bits it always did.

    active LinearLR   b * (start_factor + (end_factor - start_factor) * (t - begin) / (end - begin))
    active PolyLR     (b_begin - eta_min) * (1 - (t - begin) / (end - begin)) ** power + eta_min
    active ConstantLR b * factor                       (and b again from t = end on, as torch's ConstantLR)
    with b the group's base rate and b_begin its rate on entering the PolyLR; between and after the intervals the value
    reached at the end of the last finished interval holds, before the first one the base rate."""

    def __init__(self, sched_cfg, max_iters=None, power=0.9, eta_min=0.0):
        lone = sched_cfg is None or (len(sched_cfg) == 1 and sched_cfg[0].get('type', 'PolyLR') == 'PolyLR'
                                     and sched_cfg[0].get('begin', 0) == 0)
        entries = []
        for i, c in enumerate(sched_cfg if sched_cfg is not None else [dict(power=0.9, eta_min=0, end=80000)]):
            if not isinstance(c, dict):
                raise ValueError(f'param_scheduler[{i}] must be a dict')
            kind = c.get('type', 'PolyLR')
            if kind not in _SCHED_KEYS:
                raise ValueError(f"param_scheduler[{i}]: type={kind!r} is not supported (supported: 'LinearLR', 'PolyLR', "
                                 f"'ConstantLR')")
            if c.get('by_epoch', False if lone else True):
                raise ValueError(f'param_scheduler[{i}]: by_epoch=True is not supported (set by_epoch=False)')
            unknown = sorted(set(c) - _SCHED_COMMON - _SCHED_KEYS[kind])
            if unknown:
                raise ValueError(f'param_scheduler[{i}] (type={kind!r}): unknown key {unknown[0]!r}')
            begin = int(c.get('begin', 0))
            end = c.get('end', 80000 if lone else None)
            if lone and max_iters:
                end = max_iters                 # (a lone PolyLR spans the run: Trainer(max_iters=) sets its length)
            if end is None:
                raise ValueError(f'param_scheduler[{i}]: end is required')
            end = int(end)
            if not 0 <= begin < end:
                raise ValueError(f'param_scheduler[{i}]: needs 0 <= begin < end, got begin={begin}, end={end}')
            e = dict(type=kind, begin=begin, end=end)
            if kind == 'LinearLR':
                e.update(start_factor=float(c.get('start_factor', 1.0 / 3)), end_factor=float(c.get('end_factor', 1.0)))
                if not (0 < e['start_factor'] <= 1 and 0 <= e['end_factor'] <= 1):
                    raise ValueError(f'param_scheduler[{i}]: start_factor in (0, 1], end_factor in [0, 1]')
            elif kind == 'PolyLR':
                e.update(power=c.get('power', power), eta_min=c.get('eta_min', eta_min))
            else:
                e.update(factor=float(c.get('factor', 1.0 / 3)))
            entries.append(e)
        entries.sort(key=lambda e: e['begin'])
        for a, b in zip(entries, entries[1:]):
            if b['begin'] < a['end']:
                raise ValueError(f'param_scheduler: [{a["begin"]}, {a["end"]}) of {a["type"]} and [{b["begin"]}, {b["end"]}) of '
                                 f'{b["type"]} overlap')
        self.entries = entries
        self.lone_poly = lone
        self.end = max(e['end'] for e in entries)

    @staticmethod
    def _frac(e, t):
        return (min(t, e['end']) - e['begin']) / (e['end'] - e['begin'])

    def _walk(self, t, linear, poly, const, state):
        """run `state` through every interval entered by step t"""
        for e in self.entries:
            if t < e['begin']:
                break
            done = t >= e['end']
            if e['type'] == 'LinearLR':
                state = linear(e, e['start_factor'] + (e['end_factor'] - e['start_factor']) * self._frac(e, t))
            elif e['type'] == 'PolyLR':
                state = poly(e, state, (1.0 - self._frac(e, t)) ** e['power'])
            else:
                state = const(e, 1.0 if done else e['factor'])
        return state

    def value(self, base_lr, t):
        """the base group's rate at step t"""
        return self._walk(t, lambda e, f: base_lr * f, lambda e, b, f: (b - e['eta_min']) * f + e['eta_min'],
                          lambda e, f: base_lr * f, base_lr)

    def scalars(self, base_lr, t):
        """(A, B): a group of base rate lr_mult * base_lr runs at lr_mult * A + B at step t"""
        return self._walk(t, lambda e, f: (base_lr * f, 0.0),
                          lambda e, ab, f: (ab[0] * f, (ab[1] - e['eta_min']) * f + e['eta_min']),
                          lambda e, f: (base_lr * f, 0.0), (base_lr, 0.0))

    def state_dicts(self, base_values, last_step):
        """one dict per entry, the fields of the mmengine scheduler's state_dict()"""
        out = []
        for e in self.entries:
            d = dict(last_step=last_step, begin=e['begin'], end=e['end'], total_iters=e['end'] - e['begin'],
                     base_values=list(base_values), by_epoch=False)
            d.update({k: v for k, v in e.items() if k not in ('type', 'begin', 'end')})
            out.append(d)
        return out


# --------------------------------------------------------------------------- #
# custom_hooks = [dict(type='EMAHook', ema_type=, momentum=, update_buffers=, begin_iter=, interval=, gamma=), ...]
# --------------------------------------------------------------------------- #
_EMA_TYPES = {'ExponentialMovingAverage': set(), 'ExpMomentumEMA': {'gamma'}}
_EMA_KEYS = {'type', 'ema_type', 'momentum', 'update_buffers', 'begin_iter', 'interval', 'priority'}


def parse_ema_hook(custom_hooks):
    """the config's custom_hooks list -> None (no EMAHook in it) or dict(ema_type, momentum, gamma, update_buffers,
    begin_iter).  Hooks of other types are not this function's business and are skipped; inside the EMAHook entry every
    key is honoured or raises ValueError (DESIGN.md "Weight averaging in the optimizer step")."""
    if not custom_hooks:
        return None
    if not isinstance(custom_hooks, (list, tuple)):
        raise ValueError(f'custom_hooks must be a list of dicts, got {type(custom_hooks).__name__}')
    hooks = [h for h in custom_hooks if isinstance(h, dict) and h.get('type') == 'EMAHook']
    if not hooks:
        return None
    if len(hooks) > 1:
        raise ValueError('custom_hooks: more than one EMAHook')
    h = hooks[0]
    for key in ('strict_load', 'begin_epoch'):
        if key in h:
            raise ValueError(f'EMAHook: {key} is not supported' + (' (the schedule runs by iteration: use begin_iter)'
                                                                   if key == 'begin_epoch' else ''))
    ema_type = h.get('ema_type', 'ExponentialMovingAverage')
    if ema_type not in _EMA_TYPES:
        raise ValueError(f"EMAHook: ema_type={ema_type!r} is not supported (supported: 'ExponentialMovingAverage', "
                         f"'ExpMomentumEMA')")
    unknown = sorted(set(h) - _EMA_KEYS - _EMA_TYPES[ema_type])
    if unknown:
        raise ValueError(f'EMAHook (ema_type={ema_type!r}): unknown key {unknown[0]!r}')
    if h.get('interval', 1) != 1:
        raise ValueError(f'EMAHook: interval={h["interval"]!r} is not supported (only 1: the update is part of every '
                         f'optimizer launch)')
    momentum = h.get('momentum', 0.0002)
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0.0 < momentum < 1.0:
        raise ValueError(f'EMAHook: momentum={momentum!r} must be in (0, 1)')
    begin_iter = h.get('begin_iter', 0)
    if isinstance(begin_iter, bool) or not isinstance(begin_iter, int) or begin_iter < 0:
        raise ValueError(f'EMAHook: begin_iter={begin_iter!r} must be a non-negative integer')
    gamma = None
    if ema_type == 'ExpMomentumEMA':
        gamma = h.get('gamma', 2000)
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not gamma > 0:
            raise ValueError(f'EMAHook: gamma={gamma!r} must be > 0')
    return dict(ema_type=ema_type, momentum=float(momentum), gamma=gamma, update_buffers=bool(h.get('update_buffers', False)),
                begin_iter=begin_iter)


def ema_weight(ema, steps):
    """the averaging weight w of the update that follows `steps` finished ones (steps >= 1), formed in double"""
    m = ema['momentum']
    if ema['ema_type'] == 'ExpMomentumEMA':
        return (1.0 - m) * math.exp(-(1.0 + steps) / ema['gamma']) + m
    return m
