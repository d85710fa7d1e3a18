#!/usr/bin/env python3
"""What OhemCrossEntropy's class_weight costs on the MI355X (HIP events, median of --repeats after --warmup):

  kernels: the fused loss pair alone (ledn_ohem2_up_fwd + _bwd against ledn_ohem2_up_w_fwd + _w_bwd) on
           --batch x --height x --width labels -- by construction one more read of the uint8 label plane in the
           masked mean and a multiply per selected pixel;
  step:    the whole training step of BASELINE config C (16 x 3 x 1024 x 1024, bf16, fwd + OHEM-CE + bwd + SGD, one
           hipGraph replay per step, bench.py's model and batch) without weights and with weights on both losses.

    python tools/ohem_class_weight_bench.py [--out profiles/ohem_class_weight_bench.txt]
"""
import argparse
import os.path as osp
import statistics
import sys

import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
import led_net_amd as L  # noqa: E402
from led_net_amd import ops_train as T  # noqa: E402


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
    return f'{t[0]:8.3f} [{t[1]:.3f}, {t[2]:.3f}]'


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=1024)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=30)
    p.add_argument('--weights', default='0.8,1.2', help='class weights put on both losses')
    p.add_argument('--skip-step', action='store_true', help='time the loss kernels only')
    p.add_argument('--out')
    a = p.parse_args()
    import bench                                   # (repository root: the model and the batch of the benchmark)
    dev = torch.device('cuda:0')
    N, H, W = a.batch, a.height, a.width
    cw = [float(v) for v in a.weights.split(',')]
    lines = [f'ohem_class_weight_bench: {N} x {H} x {W}, class_weight {cw} on both losses, warmup {a.warmup}, '
             f'repeats {a.repeats} (median [min, max] ms)']

    # ---- the loss pair alone
    g = torch.Generator().manual_seed(304)
    s0 = (1.5 * torch.randn(N, H // 2, W // 2, 2, generator=g)).to(dev)
    s1 = (0.7 * torch.randn(N, H // 2, W // 2, 2, generator=g)).to(dev)
    _, lab = bench.synthetic_batch(N, H, W, dev)
    y = lab.squeeze(1).contiguous()
    cfg0, cfg1 = (0.9, 131072, 1.0), (0.9, 131072, 0.4)
    one = torch.ones(1, device=dev)
    wt = torch.tensor(cw, dtype=torch.float32, device=dev)

    def pair(cws):
        def fwd():
            return T.ohem2_up_fwd(s0, s1, y, cfg0, cfg1, 255, class_weights=cws)
        out, work = fwd()

        def bwd():
            return T.ohem2_up_bwd(s0, s1, (H, W), work, out, one, one, cfg0[2], cfg1[2], 255, class_weights=cws)
        return timed(fwd, a.warmup, a.repeats), timed(bwd, a.warmup, a.repeats)

    for rep in range(2):                           # twice, alternating: the spread of a repeat is on the page
        for name, cws in (('unweighted', (None, None)), ('weighted  ', (wt, wt))):
            f, b = pair(cws)
            lines.append(f'  pair {name} #{rep}  fwd {fmt(f)}   bwd {fmt(b)}')

    # ---- the whole step
    if not a.skip_step:
        for rep in range(2):
            for name, weights in (('unweighted', None), ('weighted  ', cw)):
                model, cfg = bench.build_model(dev, 'bf16', True)
                if weights is not None:
                    for c in cfg['model']['decode_head']['loss_decode']:
                        c['class_weight'] = list(weights)
                    torch.manual_seed(304)
                    model = L.MODELS.build(cfg['model'])
                    model.set_act_dtype(torch.bfloat16)
                    model.to(dev).train()
                img, lab = bench.synthetic_batch(N, H, W, dev)
                samples = [L.SegDataSample(gt=lab[i]) for i in range(N)]
                tr = L.Trainer(model, cfg)
                tr.capture(img, samples)
                t = timed(tr.replay, a.warmup, a.repeats)
                lines.append(f'  step {name} #{rep}  {fmt(t)}   {N / t[0] * 1e3:8.1f} images/s')
                del tr, model
                torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
