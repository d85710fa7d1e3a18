#!/usr/bin/env python3
"""What weight averaging (custom_hooks' EMAHook) costs on the MI355X (HIP events, median of --repeats after --warmup):

  launch:  over the real parameter table of the model (every parameter, ~1.5 M floats), SGD and AdamW:
             ledn_optim_step                          (no averaging)
             ledn_optim_step_ema                      (the averaged column in the same launch: what the Trainer runs)
             ledn_optim_step + ledn_ema_update        (the two-launch alternative over the same tensors)
           By bytes alone the averaged column is 8 more bytes per parameter on a launch that moves 16 (SGD) or 32
           (AdamW) -- a model; the lines this tool prints are the measurement;
  step:    the whole training step of BASELINE config C (16 x 3 x 1024 x 1024, bf16, fwd + OHEM-CE + bwd + SGD, one
           hipGraph replay per step, bench.py's model and batch) without the hook (the plain ledn_sgd_step launch: the
           step of a configuration without custom_hooks) and with EMAHook(momentum=0.0002), alternating in one process.

    python tools/ema_bench.py [--out profiles/ema_bench.txt]
"""
import argparse
import os.path as osp
import sys

import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.join(ROOT, 'tools'))
import led_net_amd as L  # noqa: E402
from led_net_amd import _lib, optim as O, ops_train as T  # noqa: E402
from clip_grad_bench import fmt, timed  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=1024)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=30)
    p.add_argument('--momentum', type=float, default=0.0002)
    p.add_argument('--skip-step', action='store_true', help='time the optimizer launches only')
    p.add_argument('--out')
    a = p.parse_args()
    import bench                                   # (repository root: the model and the batch of the benchmark)
    dev = torch.device('cuda:0')
    N, H, W = a.batch, a.height, a.width
    lines = [f'ema_bench: warmup {a.warmup}, repeats {a.repeats} (median [min, max])']

    # ---- the optimizer launches alone, over the real parameter table (every parameter; lr 0, no weight decay: the
    # parameters stay put however often the launch repeats, and so does the average)
    model, cfg = bench.build_model(dev, 'bf16', True)
    tr = L.Trainer(model, cfg)
    n = tr.flat_grad.numel()
    flat_v, flat_ema = torch.zeros_like(tr.flat_mom), torch.zeros_like(tr.flat_mom)
    vs, avgs, off = [], [], 0
    for q in tr.params:
        vs.append(flat_v[off:off + q.numel()].view_as(q))
        avgs.append(flat_ema[off:off + q.numel()].view_as(q))
        off += q.numel()
    w_dev = torch.full((1,), a.momentum, dtype=torch.float32, device=dev)
    update = T.EmaTable(avgs, [q.detach() for q in tr.params])
    lines.append(f'  parameter table: {len(tr.params)} tensors, {n} floats ({4 * n / 1e6:.2f} MB per column)')
    for kind, name, v in ((_lib.OPTIM_SGD, 'SGD  ', None), (_lib.OPTIM_ADAMW, 'AdamW', vs)):
        plain = T.OptimTable(tr.params, tr.views, tr.moms, v)
        fused = T.OptimTable(tr.params, tr.views, tr.moms, v, avgs=avgs)
        kw = dict(momentum=0.9, weight_decay=0.0)

        def two():
            plain.step(kind, 0.0, **kw)
            update.update(w_dev=w_dev)

        for rep in range(2):                       # twice, alternating: the spread of a repeat is on the page
            for what, fn in (('optim_step                  ', lambda: plain.step(kind, 0.0, **kw)),
                             ('optim_step_ema              ', lambda: fused.step(kind, 0.0, ema_dev=w_dev, **kw)),
                             ('optim_step + ema_update     ', two)):
                lines.append(f'  launch #{rep}  {name} {what} {fmt(timed(fn, a.warmup, a.repeats))}')
    del tr, plain, fused, update, model
    torch.cuda.empty_cache()

    # ---- the whole step
    if not a.skip_step:
        lines.append(f'  step: {N} x 3 x {H} x {W} bf16, one hipGraph replay per step')
        hook = O.parse_ema_hook([dict(type='EMAHook', momentum=a.momentum)])
        for rep in range(2):
            for name, ema in (('no hook (ledn_sgd_step)        ', None), (f'EMAHook momentum={a.momentum:g}', hook)):
                model, cfg = bench.build_model(dev, 'bf16', True)
                img, lab = bench.synthetic_batch(N, H, W, dev)
                samples = [L.SegDataSample(gt=lab[i]) for i in range(N)]
                tr = L.Trainer(model, cfg, ema=ema)
                tr.capture(img, samples)
                t = timed(tr.replay, a.warmup, a.repeats)
                lines.append(f'  step {name} #{rep}  {t[0]:8.3f} [{t[1]:.3f}, {t[2]:.3f}] ms   {N / t[0] * 1e3:8.1f} images/s'
                             + (f'   ema steps {tr.ema_steps}' if ema is not None else ''))
                del tr, model
                torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
