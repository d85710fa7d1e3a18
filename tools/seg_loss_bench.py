#!/usr/bin/env python3
"""What LEDHead(loss_decode=[CrossEntropyLoss, DiceLoss]) costs on the MI355X next to the default OHEM pair (HIP
events, median of --repeats after --warmup), loss kernels only, on --batch x --height x --width labels:

  ohem pair:  ledn_ohem2_up_fwd + ledn_ohem2_up_bwd (both OhemCrossEntropy losses in one launch set)
  ce + dice:  ledn_ce_loss_up_fwd + ledn_dice_loss_up_fwd, then ledn_dice_loss_up_bwd + ledn_ce_loss_up_bwd
              (the launch set of the [CE, Dice] head: each loss on its own)

Then each resize-folded launch on its own, FocalLoss and TverskyLoss next to the CrossEntropyLoss / DiceLoss launches
of the same shape (the in-tree yardstick), with the ratio to each of them:

  ce / dice / focal / tversky fwd:  ledn_{ce,dice,focal,tversky}_loss_up_fwd (pass + finish)
  ce / dice / focal / tversky bwd:  ledn_{ce,dice,focal,tversky}_loss_up_bwd

GB/s: the bytes a launch set must move at least (int64 labels and the half-size sources once per kernel that reads
them, the source gradients once) over the median time.

    python tools/seg_loss_bench.py [--out profiles/seg_loss_bench.txt]
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


def fmt(t, nbytes):
    return f'{t[0]:8.3f} [{t[1]:.3f}, {t[2]:.3f}] ms  {nbytes / t[0] / 1e6:7.0f} GB/s'


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=1024)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=30)
    p.add_argument('--out')
    a = p.parse_args()
    import bench                                   # (repository root: the batch of the benchmark)
    dev = torch.device('cuda:0')
    N, H, W = a.batch, a.height, a.width
    g = torch.Generator().manual_seed(304)
    s0 = (1.5 * torch.randn(N, H // 2, W // 2, 2, generator=g)).to(dev)
    s1 = (0.7 * torch.randn(N, H // 2, W // 2, 2, generator=g)).to(dev)
    _, lab = bench.synthetic_batch(N, H, W, dev)
    y = lab.squeeze(1).contiguous()
    one = torch.ones(1, device=dev)
    cfg0, cfg1 = (0.9, 131072, 1.0), (0.9, 131072, 0.4)
    P = N * H * W
    src, lab8 = s0.numel() * 4, P * 8
    lines = [f'seg_loss_bench: {N} x {H} x {W}, warmup {a.warmup}, repeats {a.repeats} (median [min, max] ms; GB/s = '
             f'minimum traffic / median)']

    def ohem_fwd():
        return T.ohem2_up_fwd(s0, s1, y, cfg0, cfg1, 255)
    o_out, o_work = ohem_fwd()

    def ohem_bwd():
        return T.ohem2_up_bwd(s0, s1, (H, W), o_work, o_out, one, one, cfg0[2], cfg1[2], 255)

    state = {}

    def new_fwd():
        state['ce'] = T.ce_loss_up_fwd(s0, y, loss_weight=1.0, ignore_index=255, avg_non_ignore=True)
        state['dice'] = T.dice_loss_up_fwd(s1, y, loss_weight=0.4)
    new_fwd()

    def new_bwd():
        T.dice_loss_up_bwd(s1, y, state['dice'][1], state['dice'][0], one, loss_weight=0.4)
        T.ce_loss_up_bwd(s0, y, state['ce'][1], state['ce'][0], one, loss_weight=1.0, ignore_index=255)

    # minimum traffic: ohem fwd = labels + 2 sources + 2 probability planes + uint8 labels written; its bwd reads those
    # planes and writes 2 gradients.  new fwd = 2 x (labels + source); new bwd = 2 x (labels + source + gradient)
    traffic = {'ohem fwd': lab8 + 2 * src + 9 * P, 'ohem bwd': 9 * P + 2 * src,
               'ce+dice fwd': 2 * (lab8 + src), 'ce+dice bwd': 2 * (lab8 + 2 * src)}
    for rep in range(2):                           # twice, alternating: the spread of a repeat is on the page
        res = {'ohem fwd': timed(ohem_fwd, a.warmup, a.repeats), 'ohem bwd': timed(ohem_bwd, a.warmup, a.repeats),
               'ce+dice fwd': timed(new_fwd, a.warmup, a.repeats), 'ce+dice bwd': timed(new_bwd, a.warmup, a.repeats)}
        for k, t in res.items():
            lines.append(f'  #{rep} {k:12s} {fmt(t, traffic[k])}')
        lines.append(f'  #{rep} fwd + bwd    ohem pair {res["ohem fwd"][0] + res["ohem bwd"][0]:.3f} ms   '
                     f'ce + dice {res["ce+dice fwd"][0] + res["ce+dice bwd"][0]:.3f} ms')
    # the four families launch by launch: forward = labels + source read, backward = those + the source gradient
    fams = {'ce': (T.ce_loss_up_fwd, T.ce_loss_up_bwd, dict(loss_weight=1.0, ignore_index=255, avg_non_ignore=True),
                   dict(loss_weight=1.0, ignore_index=255)),
            'dice': (T.dice_loss_up_fwd, T.dice_loss_up_bwd, dict(loss_weight=0.4), dict(loss_weight=0.4)),
            'focal': (T.focal_loss_up_fwd, T.focal_loss_up_bwd, dict(gamma=2.0, alpha=0.5), dict(gamma=2.0, alpha=0.5)),
            'tversky': (T.tversky_loss_up_fwd, T.tversky_loss_up_bwd, dict(alpha=0.3, beta=0.7, loss_weight=0.4), dict())}
    saved = {k: f[0](s0, y, **f[2]) for k, f in fams.items()}
    for rep in range(2):
        res = {}
        for k, (fwd, bwd, fkw, bkw) in fams.items():
            res[k, 'fwd'] = timed(lambda: fwd(s0, y, **fkw), a.warmup, a.repeats)
            res[k, 'bwd'] = timed(lambda: bwd(s0, y, saved[k][1], saved[k][0], one, **bkw), a.warmup, a.repeats)
        for d, nbytes in (('fwd', lab8 + src), ('bwd', lab8 + 2 * src)):
            for k in fams:
                t = res[k, d]
                ratio = '' if k in ('ce', 'dice') else \
                    f'  x{t[0] / res["ce", d][0]:.2f} of ce, x{t[0] / res["dice", d][0]:.2f} of dice'
                lines.append(f'  #{rep} {k + " " + d:12s} {fmt(t, nbytes)}{ratio}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
