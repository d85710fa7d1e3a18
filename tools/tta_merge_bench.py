#!/usr/bin/env python3
"""Fused merge kernels against the composition they replace, at the original resolution (HIP events, median of
--repeats after --warmup):

  tta:   12 views (the cityscapes ratios x two flips) of a 1024 x 2048 x 19 image
         (a) ops.tta_accumulate per view                       [2 passes over the accumulator per view]
         (b) ops.bilinear(nchw=True) + torch.softmax + add_ per view, argmax at the end   [about 6 passes]
  slide: 1024 x 2048 canvas, 1024 x 1024 windows, stride 768
         (a) ops.slide_accumulate per window (planar crops, as slide_inference; NHWC crops timed too) + ops.slide_finish
         (b) F.pad + add per window, count matrix, divide, argmax

    python tools/tta_merge_bench.py [--out profiles/tta_merge_bench.txt]
"""
import argparse
import os.path as osp
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from led_net_amd import ops  # noqa: E402

RATIOS = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]


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
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=2048)
    p.add_argument('--classes', type=int, default=19)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=30)
    p.add_argument('--out')
    a = p.parse_args()
    dev = torch.device('cuda:0')
    H, W, C = a.height, a.width, a.classes
    g = torch.Generator().manual_seed(304)
    views = [(torch.randn((int(H * r + 0.5), int(W * r + 0.5), C), generator=g).to(dev), flip)
             for r in RATIOS for flip in (None, 'horizontal')]
    K = len(views)
    acc = torch.empty((C, H, W), device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    plane = C * H * W * 4
    src_bytes = sum(v.numel() * 4 for v, _ in views)

    def fused():
        for k, (v, flip) in enumerate(views):
            ops.tta_accumulate(v, acc, first=k == 0, last=k == K - 1, K=K, flip=flip, mask=mask if k == K - 1 else None)

    def composed():
        total = None
        for v, flip in views:
            lg = v.flip(dims=(1,)).contiguous() if flip else v
            pr = torch.softmax(ops.bilinear(lg[None], (H, W), nchw=True)[0], dim=0)
            total = pr if total is None else total.add_(pr)
        total /= K
        return total.argmax(0)

    lines = [f'tta_merge_bench: {K} views -> {C} x {H} x {W} f32, warmup {a.warmup}, repeats {a.repeats} (median [min, max] ms)']
    fa, fb = timed(fused, a.warmup, a.repeats), timed(composed, a.warmup, a.repeats)
    by_a = src_bytes + plane * (2 * K - 1) + H * W                      # first view writes only
    by_b = src_bytes * 2 + plane * (4 * K + 3 * (K - 1) + 2 + 1)        # flip copy; resize w, softmax r+w, add r+r+w, /K r+w, argmax r
    lines.append(f'  tta   fused    {fa[0]:8.3f} [{fa[1]:.3f}, {fa[2]:.3f}]  {by_a / 1e9:6.2f} GB  {by_a / fa[0] / 1e9:5.2f} TB/s')
    lines.append(f'  tta   composed {fb[0]:8.3f} [{fb[1]:.3f}, {fb[2]:.3f}]  {by_b / 1e9:6.2f} GB  {by_b / fb[0] / 1e9:5.2f} TB/s')
    lines.append(f'  tta   speed-up {fb[0] / fa[0]:.2f}x')

    ch, cw, sh, sw = 1024, 1024, 768, 768
    boxes = []
    for hi in range(max(H - ch + sh - 1, 0) // sh + 1):
        for wi in range(max(W - cw + sw - 1, 0) // sw + 1):
            y2, x2 = min(hi * sh + ch, H), min(wi * sw + cw, W)
            boxes.append((max(y2 - ch, 0), y2, max(x2 - cw, 0), x2))
    crops = [torch.randn((1, y2 - y1, x2 - x1, C), generator=g).to(dev) for y1, y2, x1, x2 in boxes]
    crops_nchw = [c.permute(0, 3, 1, 2).contiguous() for c in crops]     # what the parent's encode_decode returns
    rowcnt, colcnt = torch.zeros(H, dtype=torch.int32), torch.zeros(W, dtype=torch.int32)
    for y1, y2, x1, x2 in boxes:
        rowcnt[y1:y2] += 1 if x1 == 0 else 0
        colcnt[x1:x2] += 1 if y1 == 0 else 0
    canvas = torch.empty((1, C, H, W), device=dev)

    def slide_fused():
        canvas.zero_()
        for (y1, y2, x1, x2), c in zip(boxes, crops_nchw):          # planar window logits: what slide_inference launches
            ops.slide_accumulate(canvas, c, y1, x1, planar=True)
        return ops.slide_finish(canvas, rowcnt, colcnt)

    def slide_fused_nhwc():
        canvas.zero_()
        for (y1, y2, x1, x2), c in zip(boxes, crops):
            ops.slide_accumulate(canvas, c, y1, x1)
        return ops.slide_finish(canvas, rowcnt, colcnt)

    def slide_composed():
        preds = torch.zeros((1, C, H, W), device=dev)
        count = torch.zeros((1, 1, H, W), device=dev)
        for (y1, y2, x1, x2), c in zip(boxes, crops_nchw):
            preds += F.pad(c, (x1, W - x2, y1, H - y2))
            count[:, :, y1:y2, x1:x2] += 1
        return (preds / count).argmax(1)

    sa, sb = timed(slide_fused, a.warmup, a.repeats), timed(slide_composed, a.warmup, a.repeats)
    sn = timed(slide_fused_nhwc, a.warmup, a.repeats)
    crop_bytes = sum(c.numel() * 4 for c in crops)
    by_a = plane + 3 * crop_bytes + 2 * plane + H * W
    by_b = plane + len(boxes) * (crop_bytes // len(boxes) + plane + 3 * plane) + 3 * plane
    lines.append(f'  slide fused    {sa[0]:8.3f} [{sa[1]:.3f}, {sa[2]:.3f}]  {by_a / 1e9:6.2f} GB  {by_a / sa[0] / 1e9:5.2f} TB/s  ({len(boxes)} windows)')
    lines.append(f'  slide fused/nhwc crops {sn[0]:8.3f} [{sn[1]:.3f}, {sn[2]:.3f}]')
    lines.append(f'  slide composed {sb[0]:8.3f} [{sb[1]:.3f}, {sb[2]:.3f}]  {by_b / 1e9:6.2f} GB  {by_b / sb[0] / 1e9:5.2f} TB/s')
    lines.append(f'  slide speed-up {sb[0] / sa[0]:.2f}x')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
