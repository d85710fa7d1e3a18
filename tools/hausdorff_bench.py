#!/usr/bin/env python3
"""What a HuasdorffDisstanceLoss entry of LEDHead costs on the MI355X (HIP events, median of --repeats after --warmup),
loss kernels only, on --batch x --classes x --height x --width full-resolution logits, for two label / prediction sets:

  blobs:  a few filled rectangles and discs per image, the prediction the same shapes moved by a few pixels
  corner: the row search's worst case -- labels and prediction all foreground except ONE corner pixel per image, so that
          every pixel walks to the far end of its row

  hausdorff fwd:  ledn_hausdorff_loss_fwd -- column pass (both masks), row pass (both maps), loss, finish
  hausdorff bwd:  ledn_hausdorff_loss_bwd -- one streaming kernel
  edt_sq:         ledn_edt_sq on the label mask alone (one column pass, one row pass)
  ce fwd/bwd:     ledn_ce_loss_fwd / _bwd on the same logits (the in-tree yardstick)

Next to the times: the bytes the passes must move at least.  Per pixel, forward: column pass reads the logits and the
label (4 C + 8) and writes, re-reads and re-writes two int32 maps (24), row pass reads and writes them (16), loss pass
reads logits, label and both maps and writes D (4 C + 8 + 12); backward: logits, label, D in, gradient out (8 C + 12).
Per-kernel times come from running this tool under a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/hausdorff_bench.py ...).

    python tools/hausdorff_bench.py [--classes 2] [--out profiles/hausdorff_bench.txt]
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


def blobs(N, H, W, g):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    y = torch.zeros((N, H, W), dtype=torch.int64)
    for b in range(N):
        for k in range(4):
            cy, cx = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
            r = int(torch.randint(min(H, W) // 10, min(H, W) // 4, (1,), generator=g))
            m = ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r) if k % 2 else (((yy - cy).abs() <= r) & ((xx - cx).abs() <= r))
            y[b][m] = 1
    return y


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--classes', type=int, default=2)
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=1024)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--repeats', type=int, default=10)
    p.add_argument('--out')
    a = p.parse_args()
    dev = torch.device('cuda:0')
    N, C, H, W = a.batch, a.classes, a.height, a.width
    g = torch.Generator().manual_seed(304)
    P = N * H * W
    fwd_bytes = ((4 * C + 8) + 24 + 16 + (4 * C + 8 + 12)) * P
    bwd_bytes = (8 * C + 12) * P
    lines = [f'hausdorff_bench: {N} x {C} x {H} x {W}, warmup {a.warmup}, repeats {a.repeats} (median [min, max] ms); minimum '
             f'traffic forward {fwd_bytes / 1e9:.2f} GB, backward {bwd_bytes / 1e9:.2f} GB']
    one = torch.ones(1, device=dev)
    for name in ('blobs', 'corner'):
        if name == 'blobs':
            y = blobs(N, H, W, g)
            pred = torch.roll(y, shifts=(5, -7), dims=(1, 2))
            y[:, :8, :] = 255
        else:
            y = torch.ones((N, H, W), dtype=torch.int64)
            y[:, H - 1, 0] = 0
            pred = y.clone()
        x = 0.5 * torch.randn(N, H, W, C, generator=g)
        x.scatter_add_(3, pred.unsqueeze(3), torch.full((N, H, W, 1), 4.0))
        x, y = x.to(dev), y.to(dev)
        mask = ((y != 0) & (y != 255)).to(torch.uint8)
        out, work = T.hausdorff_loss_fwd(x, y, loss_weight=0.02)
        ce_out, ce_work = T.ce_loss_fwd(x, y, avg_non_ignore=True)
        lines.append(f'  {name}: work buffer {work.numel() * 4 / 2**20:.0f} MiB, loss {float(out[0]):.6g} acc {float(out[1]):.3f}, '
                     f'largest D {int(work[4:4 + P].view(torch.int32).max())}')
        for rep in range(2):
            f = timed(lambda: T.hausdorff_loss_fwd(x, y, loss_weight=0.02), a.warmup, a.repeats)
            b = timed(lambda: T.hausdorff_loss_bwd(x, y, work, out, one), a.warmup, a.repeats)
            e = timed(lambda: T.edt_sq(mask), a.warmup, a.repeats)
            cf = timed(lambda: T.ce_loss_fwd(x, y, avg_non_ignore=True), a.warmup, a.repeats)
            cb = timed(lambda: T.ce_loss_bwd(x, y, ce_work, ce_out, one), a.warmup, a.repeats)
            lines.append(f'  #{rep} {name} hausdorff fwd {f[0]:9.3f} [{f[1]:.3f}, {f[2]:.3f}] ms   {fwd_bytes / f[0] / 1e6:7.0f} GB/s of '
                         f'minimum traffic = {fwd_bytes / f[0] / 1e6 / 8000:.1%} of 8 TB/s')
            lines.append(f'  #{rep} {name} hausdorff bwd {b[0]:9.3f} [{b[1]:.3f}, {b[2]:.3f}] ms   {bwd_bytes / b[0] / 1e6:7.0f} GB/s')
            lines.append(f'  #{rep} {name} edt_sq        {e[0]:9.3f} [{e[1]:.3f}, {e[2]:.3f}] ms')
            lines.append(f'  #{rep} {name} ce fwd        {cf[0]:9.3f} [{cf[1]:.3f}, {cf[2]:.3f}] ms   ce bwd {cb[0]:9.3f} '
                         f'[{cb[1]:.3f}, {cb[2]:.3f}] ms')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
