#!/usr/bin/env python3
"""What a LovaszLoss entry of LEDHead costs on the MI355X (HIP events, median of --repeats after --warmup), loss kernels
only, on --batch x --classes x --height x --width full-resolution logits:

  lovasz fwd:  ledn_lovasz_loss_fwd -- count, then per class build + 4 x (hist, scan, scatter) + fgtot, scan, loss,
               accumulate, then the finish (csrc/lovasz.hip)
  lovasz bwd:  ledn_lovasz_loss_bwd -- one streaming kernel over the stored logit gradient
  ce fwd/bwd:  ledn_ce_loss_fwd / _bwd on the same logits (the in-tree yardstick)

Next to the times: the bytes the sort must move at least (per class and pass: histogram read 4 B, scatter read 8 B +
write 8 B per pixel = 20 B) and the rate that makes of the forward.  Per-kernel times come from running this tool under
a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/lovasz_bench.py ...).

    python tools/lovasz_bench.py [--classes 2] [--per-image] [--mode present] [--out profiles/lovasz_bench.txt]
"""
import argparse
import os.path as osp
import statistics
import sys

import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--classes', type=int, default=2)
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=1024)
    p.add_argument('--mode', default='present', choices=['present', 'all'])
    p.add_argument('--per-image', action='store_true')
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--repeats', type=int, default=10)
    p.add_argument('--out')
    a = p.parse_args()
    dev = torch.device('cuda:0')
    N, C, H, W = a.batch, a.classes, a.height, a.width
    g = torch.Generator().manual_seed(304)
    x = (1.5 * torch.randn(N, H, W, C, generator=g)).to(dev)
    y = torch.randint(0, C, (N, H, W), generator=g)
    y[torch.rand((N, H, W), generator=g) < 0.05] = 255
    y = y.to(dev)
    one = torch.ones(1, device=dev)
    P = N * H * W
    kw = dict(classes=a.mode, per_image=a.per_image, loss_weight=0.4)
    out, work = T.lovasz_loss_fwd(x, y, **kw)
    ce_out, ce_work = T.ce_loss_fwd(x, y, avg_non_ignore=True)
    ncls = C if a.mode == 'all' else int(torch.unique(y[y != 255]).numel())
    sort_bytes = ncls * 4 * 20 * P
    rest_bytes = ncls * ((4 * C + 8 + 8) * P + 4 * P + (8 + 4) * P + (4 * C + 8 + 4 + 8 * C) * P) + (4 * C + 8) * P
    lines = [f'lovasz_bench: {N} x {C} x {H} x {W}, classes={a.mode!r} ({ncls} computed), per_image={a.per_image}, warmup '
             f'{a.warmup}, repeats {a.repeats} (median [min, max] ms)',
             f'  work buffer {work.numel() * 4 / 2**20:.0f} MiB; minimum traffic: sort {sort_bytes / 1e9:.2f} GB '
             f'({ncls} classes x 4 passes x 20 B x {P} pixels), build + scan + loss + accumulate {rest_bytes / 1e9:.2f} GB']
    for rep in range(2):
        f = timed(lambda: T.lovasz_loss_fwd(x, y, **kw), a.warmup, a.repeats)
        b = timed(lambda: T.lovasz_loss_bwd(x, y, work, out, one), a.warmup, a.repeats)
        cf = timed(lambda: T.ce_loss_fwd(x, y, avg_non_ignore=True), a.warmup, a.repeats)
        cb = timed(lambda: T.ce_loss_bwd(x, y, ce_work, ce_out, one), a.warmup, a.repeats)
        lines.append(f'  #{rep} lovasz fwd {f[0]:9.3f} [{f[1]:.3f}, {f[2]:.3f}] ms   {(sort_bytes + rest_bytes) / f[0] / 1e6:7.0f} GB/s '
                     f'of minimum traffic = {(sort_bytes + rest_bytes) / f[0] / 1e6 / 8000:.1%} of 8 TB/s')
        lines.append(f'  #{rep} lovasz bwd {b[0]:9.3f} [{b[1]:.3f}, {b[2]:.3f}] ms   {8 * C * P / b[0] / 1e6:7.0f} GB/s')
        lines.append(f'  #{rep} ce fwd     {cf[0]:9.3f} [{cf[1]:.3f}, {cf[2]:.3f}] ms   ce bwd {cb[0]:9.3f} [{cb[1]:.3f}, {cb[2]:.3f}] ms')
    lines.append(f'  loss {float(out[0]):.6f} acc {float(out[1]):.3f} divisor {float(out[2]):.0f} valid {float(out[3]):.0f}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
