#!/usr/bin/env python3
"""What the generalised optimizer step (ledn_optim_step: AdamW, paramwise multipliers, scheduler lists) costs on the
MI355X as a standalone launch next to ledn_sgd_step (HIP events, median of --repeats after --warmup), over the real
parameter table of the model (the Trainer's flat buffers, ~1.5 M floats), and the achieved GB/s on the bytes the step has
to move: 16 B per element for SGD (p, g, m read; p, m, g written: 24 B touched, 16 B is the project's accounting of the
existing launch and is kept for comparison) and 32 B per element for AdamW (p, g, m, v read and written).

    python tools/optim_step_bench.py [--out profiles/optim_step_bench.txt]

--guard adds the step guard's launches (the finite pass, the verdict, ledn_optim_step_guarded) to the list.

--trace sgd|adamw|adamw-clip runs nothing but --steps eager training steps (2 x 3 x 320 x 320, f32) for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/optim_step_bench.py --trace adamw): `steps` launches of optim_kernel
where the plain configuration shows `steps` of sgd_kernel -- the step still ends in ONE optimizer launch, plus the norm
pass (grad_norm_partials_kernel) when clipping by norm.
"""
import argparse
import os.path as osp
import statistics
import sys

import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
import led_net_amd as L  # noqa: E402
from led_net_amd import _lib, ops_train as T  # noqa: E402


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def fmt(t, nbytes):
    return f'{t[0] * 1e3:9.1f} [{t[1] * 1e3:.1f}, {t[2] * 1e3:.1f}] us  {nbytes / (t[0] * 1e-3) / 1e9:8.1f} GB/s'


def trace(mode, steps):
    dev = torch.device('cuda:0')
    torch.manual_seed(304)
    cfg = L.load_config(osp.join(ROOT, 'tests', 'data', 'lednet_test_config.py'))
    if mode != 'sgd':
        cfg['optim_wrapper'] = dict(type='OptimWrapper', optimizer=dict(type='AdamW', lr=1e-3, weight_decay=0.01),
                                    paramwise_cfg=dict(norm_decay_mult=0.),
                                    clip_grad=dict(max_norm=1.0) if mode == 'adamw-clip' else None)
        cfg['param_scheduler'] = [dict(type='LinearLR', start_factor=1e-3, by_epoch=False, begin=0, end=5),
                                  dict(type='PolyLR', power=0.9, eta_min=0, begin=5, end=1000, by_epoch=False)]
    model = L.MODELS.build(cfg['model']).to(dev)
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (2, 3, 320, 320), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 2, (2, 1, 320, 320), dtype=torch.int64, generator=g).to(dev)
    samples = [L.SegDataSample(gt=lab[i]) for i in range(2)]
    tr = L.Trainer(model, cfg, max_iters=1000)
    for _ in range(steps):
        out = tr.train_step(img, samples)
    torch.cuda.synchronize()
    print(f'trace: {steps} eager steps, {mode}:', {k: float(v.float().reshape(-1)[0]) for k, v in out.items()})


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=30)
    p.add_argument('--trace', choices=['sgd', 'adamw', 'adamw-clip'], help='only run --steps eager steps (for a kernel trace)')
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--guard', action='store_true',
                   help='add the step guard: finite pass + verdict + ledn_optim_step_guarded next to ledn_optim_step, SGD and AdamW')
    p.add_argument('--out')
    a = p.parse_args()
    if a.trace:
        return trace(a.trace, a.steps)
    import bench                                   # (repository root: the model of the benchmark)
    dev = torch.device('cuda:0')
    lines = [f'optim_step_bench: warmup {a.warmup}, repeats {a.repeats} (median [min, max]); lr 0, no weight decay: the '
             f'parameters stay put however often a launch repeats']
    model, cfg = bench.build_model(dev, 'bf16', True)
    tr = L.Trainer(model, cfg)
    n = tr.flat_grad.numel()
    flat_v = torch.zeros_like(tr.flat_mom)
    vs, off = [], 0
    for q in tr.params:
        vs.append(flat_v[off:off + q.numel()].view_as(q))
        off += q.numel()
    sgd = T.SgdTable(tr.params, tr.views, tr.moms)
    mults = [(10.0 if 'decode_head' in name else 1.0, 0.0 if q.ndim == 1 else 1.0) for name, q in zip(tr.names, tr.params)]
    gsgd = T.OptimTable(tr.params, tr.views, tr.moms, None, [m[0] for m in mults], [m[1] for m in mults])
    adamw = T.OptimTable(tr.params, tr.views, tr.moms, vs, [m[0] for m in mults], [m[1] for m in mults])
    aligned = sum(all(t.data_ptr() % 16 == 0 for t in ts) and ts[0].numel() >= 4
                  for ts in zip(tr.params, tr.views, tr.moms, vs))
    nvec = sum(ts[0].numel() for ts in zip(tr.params, tr.views, tr.moms, vs)
               if all(t.data_ptr() % 16 == 0 for t in ts) and ts[0].numel() >= 4)
    lines.append(f'  parameter table: {sgd.n} tensors, {n} floats; {aligned} tensors ({nvec} floats) on the 16-byte path')
    clip = T.GradClip(dev, n, _lib.NORM_L2, max_norm=1.0)
    sched = torch.tensor(T.optim_scalars(0.0, 0.0, (0.9, 0.999), 10), dtype=torch.float32, device=dev)

    def adamw_clip():
        clip.norm_pass(tr.flat_grad)
        adamw.step(_lib.OPTIM_ADAMW, 0.0, t=10, clip=clip)
    cases = [('ledn_sgd_step                          ', lambda: sgd.step(0.0, 0.9, 0.0, 1.0), 16),
             ('ledn_optim_step SGD + paramwise        ', lambda: gsgd.step(_lib.OPTIM_SGD, 0.0, momentum=0.9), 16),
             ('ledn_optim_step AdamW + paramwise      ', lambda: adamw.step(_lib.OPTIM_ADAMW, 0.0, t=10), 32),
             ('ledn_optim_step AdamW, scalars on device', lambda: adamw.step(_lib.OPTIM_ADAMW, 0.0, t=10, sched_dev=sched), 32),
             ('norm pass + ledn_optim_step AdamW (l2) ', adamw_clip, 36)]
    if a.guard:
        # the gradient stays finite (zeros): every guarded launch is an applied step, as every step of a healthy run is
        guard = T.StepGuard(dev, adamw.n)

        def guarded(table, kind, **kw):
            def run():
                guard.finite_pass(table)
                guard.verdict(table, (0.9, 0.999), 0)
                table.step(kind, 0.0, guard=guard, **kw)
            return run
        cases += [('finite pass alone                      ', lambda: guard.finite_pass(adamw), 4),
                  ('finite pass + verdict                  ', lambda: (guard.finite_pass(adamw), guard.verdict(adamw)), 4),
                  ('guard + ledn_optim_step_guarded SGD    ', guarded(gsgd, _lib.OPTIM_SGD, momentum=0.9), 20),
                  ('guard + ledn_optim_step_guarded AdamW  ', guarded(adamw, _lib.OPTIM_ADAMW), 36)]
    for rep in range(2):                           # twice, alternating: the spread of a repeat is on the page
        for name, fn, per in cases:
            lines.append(f'  launch #{rep}  {name} {fmt(timed(fn, a.warmup, a.repeats), per * n)}  ({per} B/element)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
