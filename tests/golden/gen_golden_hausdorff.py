#!/usr/bin/env python3
"""Golden vectors for HuasdorffDisstanceLoss: the reference's own class (mmseg/models/losses/huasdorff_distance_loss.py:
77-160, with scipy's distance_transform_edt under it) and its accuracy, IMPORTED from the reference checkout
(gen_golden_class_weight.REF) and run on seeded logits and labels.  Only data is written
(tests/golden/g25_hausdorff_*.npz: in/score, in/target, out/loss, out/acc, gin/score (d score by autograd), meta with the
class name, the constructor kwargs and the call's ignore_index); re-run: python tests/golden/gen_golden_hausdorff.py

Every fixture has at most 8 192 pixels.  Labels are a few filled shapes (ellipses and rectangles), the 255 labels one
filled rectangle of about a tenth of the image, and the logits follow the same shapes moved by a few pixels plus noise, so
that both distance maps reach a good part of the image size.  The reference takes the argmax of the f32 softmax, the
kernels the first maximum of the logits: a fixture whose two disagree anywhere (probabilities rounded to a tie) is
refused here.

Import plumbing: as gen_golden_seg_losses.py / gen_golden_lovasz.py.
"""
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_class_weight import REF  # noqa: E402
from gen_golden_seg_losses import install_all, save  # noqa: E402


def shapes(n, h, w, g, classes=(1,), count=3):
    """[n,h,w] int64: `count` filled ellipses / rectangles per image, labelled with `classes` in turn, on background 0"""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    out = torch.zeros((n, h, w), dtype=torch.int64)
    for b in range(n):
        for k in range(count):
            cy, cx = (torch.rand(2, generator=g) * torch.tensor([h, w])).tolist()
            ry, rx = ((0.12 + 0.2 * torch.rand(2, generator=g)) * torch.tensor([h, w])).tolist()
            if k % 2 == 0:
                m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            else:
                m = ((yy - cy).abs() <= ry) & ((xx - cx).abs() <= rx)
            out[b][m] = classes[(b + k) % len(classes)]
    return out


def ignored_rectangle(tgt, g, share=0.1):
    """one filled rectangle of 255 per image, about `share` of the pixels"""
    n, h, w = tgt.shape
    rh, rw = max(1, round(h * share ** 0.5)), max(1, round(w * share ** 0.5))
    for b in range(n):
        y0 = int(torch.randint(0, h - rh + 1, (1,), generator=g))
        x0 = int(torch.randint(0, w - rw + 1, (1,), generator=g))
        tgt[b, y0:y0 + rh, x0:x0 + rw] = 255
    return tgt


def logits_for(pred_label, c, g, margin=2.0, noise=0.6):
    """[n,c,h,w] f32 whose argmax is `pred_label` except where the noise wins (rare at this margin)"""
    n, h, w = pred_label.shape
    x = noise * torch.randn((n, c, h, w), generator=g)
    x.scatter_add_(1, pred_label.unsqueeze(1), torch.full((n, 1, h, w), margin))
    return x


def main():
    install_all()
    assert os.path.isdir(REF)
    from mmseg.models.losses.huasdorff_distance_loss import HuasdorffDisstanceLoss
    from mmseg.models.losses.accuracy import accuracy
    # name, kwargs, (N, C, H, W), special
    cases = [
        ('g25_hausdorff_blobs', dict(), (2, 2, 64, 64), None),
        ('g25_hausdorff_sum_w04', dict(loss_weight=0.4, reduction='sum'), (2, 2, 64, 64), None),
        ('g25_hausdorff_c5', dict(), (2, 5, 32, 32), None),
        ('g25_hausdorff_48x40', dict(reduction='none'), (2, 2, 48, 40), None),
        # image 0: the label is all foreground; image 1: the argmax is all foreground; image 2: no foreground anywhere
        ('g25_hausdorff_full_and_empty', dict(), (3, 2, 48, 40), 'full_and_empty'),
    ]
    g = torch.Generator().manual_seed(2500)
    for name, kw, shp, special in cases:
        n, c, h, w = shp
        assert n * h * w <= 8192
        cls = tuple(range(1, c))
        tgt = shapes(n, h, w, g, cls)
        pred = torch.roll(shapes(n, h, w, g, cls, count=1) | tgt, shifts=(3, -4), dims=(1, 2)) if c == 2 else \
            torch.roll(tgt, shifts=(3, -4), dims=(1, 2))
        if special == 'full_and_empty':
            tgt[0] = 1
            pred[1] = 1
            tgt[2] = 0
            pred[2] = 0
        else:
            tgt = ignored_rectangle(tgt, g)
        # (the special images keep a margin the noise cannot cross: an all-foreground argmax must stay one)
        score = logits_for(pred, c, g, margin=6.0 if special else 2.0)
        assert torch.equal(score.argmax(1), torch.softmax(score, 1).argmax(1)), 'softmax rounded two logits to a tie'
        if special:
            am = score.argmax(1)
            assert bool((am[1] != 0).all()) and bool((am[2] == 0).all()) and bool((tgt[0] == 1).all())
        score.requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            crit = HuasdorffDisstanceLoss(**kw)
        loss = crit(score, tgt, ignore_index=255)
        loss.backward()
        acc = accuracy(score.detach(), tgt, ignore_index=255)
        save(name, {'score': score.detach(), 'target': tgt}, {'loss': loss.detach(), 'acc': acc}, {'score': score.grad},
             dict(kind='HuasdorffDisstanceLoss', kwargs=kw, ignore_index=255))


if __name__ == '__main__':
    main()
