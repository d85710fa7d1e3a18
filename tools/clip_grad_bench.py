#!/usr/bin/env python3
"""What gradient clipping (optim_wrapper.clip_grad) costs on the MI355X (HIP events, median of --repeats after --warmup):

  launch:  over the real parameter table of the model (the Trainer's flat gradient buffer, ~1.5 M floats): the plain
           ledn_sgd_step launch against the norm pass + ledn_sgd_step_clip (L2 and inf), and against clip by value
           (one launch, no norm pass).  By design one more 6 MB read and one more launch boundary;
  step:    the whole training step of BASELINE config C (16 x 3 x 1024 x 1024, bf16, fwd + OHEM-CE + bwd + SGD, one
           hipGraph replay per step, bench.py's model and batch) with clip_grad=None and with
           clip_grad=dict(max_norm=1.0), alternating in one process.

    python tools/clip_grad_bench.py [--out profiles/clip_grad_bench.txt]

--trace off|on runs nothing but --steps eager training steps (2 x 3 x 320 x 320, f32) with clipping off / on, for a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/clip_grad_bench.py --trace on): the clipped run shows
`steps` launches of grad_norm_partials_kernel and of sgd_clip_kernel where the other shows `steps` of sgd_kernel, i.e.
one launch more per step.
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


def fmt(t):
    return f'{t[0] * 1e3:9.1f} [{t[1] * 1e3:.1f}, {t[2] * 1e3:.1f}] us'


def trace(mode, steps):
    dev = torch.device('cuda:0')
    torch.manual_seed(304)
    cfg = L.load_config(osp.join(ROOT, 'tests', 'data', 'lednet_test_config.py'))
    model = L.MODELS.build(cfg['model']).to(dev)
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (2, 3, 320, 320), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 2, (2, 1, 320, 320), dtype=torch.int64, generator=g).to(dev)
    samples = [L.SegDataSample(gt=lab[i]) for i in range(2)]
    tr = L.Trainer(model, cfg, max_iters=1000, clip_grad=dict(max_norm=1.0) if mode == 'on' else None)
    for _ in range(steps):
        out = tr.train_step(img, samples)
    torch.cuda.synchronize()
    print(f'trace: {steps} eager steps, clip_grad {mode}:', {k: float(v.float().reshape(-1)[0]) for k, v in out.items()})


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=1024)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=30)
    p.add_argument('--max-norm', type=float, default=1.0)
    p.add_argument('--skip-step', action='store_true', help='time the optimizer launches only')
    p.add_argument('--trace', choices=['off', 'on'], help='only run --steps eager steps (for a kernel trace)')
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--out')
    a = p.parse_args()
    if a.trace:
        return trace(a.trace, a.steps)
    import bench                                   # (repository root: the model and the batch of the benchmark)
    dev = torch.device('cuda:0')
    N, H, W = a.batch, a.height, a.width
    lines = [f'clip_grad_bench: warmup {a.warmup}, repeats {a.repeats} (median [min, max])']

    # ---- the optimizer launches alone, over the real parameter table (every parameter; lr 0, no weight decay: the
    # parameters stay put however often the launch repeats)
    model, cfg = bench.build_model(dev, 'bf16', True)
    tr = L.Trainer(model, cfg)
    table = T.SgdTable(tr.params, tr.views, tr.moms)
    n = tr.flat_grad.numel()
    lines.append(f'  parameter table: {table.n} tensors, {n} floats ({4 * n / 1e6:.2f} MB of gradients), '
                 f'{T.norm_partials_count(n)} norm partials')
    clips = {'l2 ': T.GradClip(dev, n, _lib.NORM_L2, max_norm=a.max_norm),
             'inf': T.GradClip(dev, n, _lib.NORM_INF, max_norm=a.max_norm),
             'val': T.GradClip(dev, n, _lib.NORM_NONE, clip_value=a.max_norm)}

    def plain():
        table.step(0.0, 0.9, 0.0, 1.0)

    def clipped(c):
        def fn():
            c.norm_pass(tr.flat_grad)
            table.step(0.0, 0.9, 0.0, 1.0, clip=c)
        return fn

    for rep in range(2):                           # twice, alternating: the spread of a repeat is on the page
        lines.append(f'  launch #{rep}  sgd_step                        {fmt(timed(plain, a.warmup, a.repeats))}')
        for name, c in clips.items():
            what = 'sgd_step_clip (by value)       ' if name == 'val' else f'norm pass + sgd_step_clip ({name})'
            lines.append(f'  launch #{rep}  {what} {fmt(timed(clipped(c), a.warmup, a.repeats))}')
        lines.append(f'  launch #{rep}  norm pass alone (l2)            '
                     f'{fmt(timed(lambda: clips["l2 "].norm_pass(tr.flat_grad), a.warmup, a.repeats))}')
    del tr, table, model
    torch.cuda.empty_cache()

    # ---- the whole step
    if not a.skip_step:
        lines.append(f'  step: {N} x 3 x {H} x {W} bf16, one hipGraph replay per step')
        for rep in range(2):
            for name, clip in (('clip_grad=None         ', None), (f'clip_grad max_norm={a.max_norm:g}', dict(max_norm=a.max_norm))):
                model, cfg = bench.build_model(dev, 'bf16', True)
                img, lab = bench.synthetic_batch(N, H, W, dev)
                samples = [L.SegDataSample(gt=lab[i]) for i in range(N)]
                tr = L.Trainer(model, cfg, clip_grad=clip)
                tr.capture(img, samples)
                t = timed(tr.replay, a.warmup, a.repeats)
                extra = ''
                if clip is not None:
                    extra = f'   grad_norm {float(tr._static_out["grad_norm"]):.4g} coef {float(tr.clip.coef):.4g}'
                lines.append(f'  step {name} #{rep}  {t[0]:8.3f} [{t[1]:.3f}, {t[2]:.3f}] ms   {N / t[0] * 1e3:8.1f} images/s{extra}')
                del tr, model
                torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
