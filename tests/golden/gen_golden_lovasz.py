#!/usr/bin/env python3
"""Golden vectors for LovaszLoss: the reference's own class (mmseg/models/losses/lovasz_loss.py:225-323) and its
accuracy, IMPORTED from the reference checkout (gen_golden_class_weight.REF) and run on seeded logits and labels.  Only
data is written (tests/golden/g24_lovasz_*.npz: in/score, in/target, out/loss, out/acc, gin/score (d score by
autograd), meta with the class name, the constructor kwargs and the call's ignore_index);
re-run: python tests/golden/gen_golden_lovasz.py

Every fixture has at most 8 192 pixels.  Inside a run of EQUAL errors the order of torch.sort is arbitrary and every order
gives another (valid) subgradient, so a fixture whose f32 errors tie would pin the reference's accident: a pixel whose
error in some class equals another pixel's bit for bit is re-drawn until no two are equal (a handful per fixture: a few
thousand f32 values in [0.5, 1) collide at random).

Import plumbing (as gen_golden_seg_losses.py): parent packages are empty modules whose __path__ points at the reference
directories; NAME-ONLY stand-ins for mmseg.registry.MODELS and mmengine.fileio.load, and a freshly written
mmengine.utils.is_list_of (the constructor calls it on a `classes` list).
"""
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_class_weight import REF, _pkg, sibling_class_weight  # noqa: E402
from gen_golden_seg_losses import install_all, save  # noqa: E402


def is_list_of(seq, expected_type):
    """True for a list whose items all have the expected type"""
    return isinstance(seq, list) and all(isinstance(item, expected_type) for item in seq)


def install_more():
    install_all()
    sys.modules['mmengine'].utils = _pkg('mmengine.utils', is_list_of=is_list_of)


def tied_pixels(score, tgt):
    """[N,H,W] bool: valid pixels whose f32 error |fg - softmax(score)_c| equals another valid pixel's in some class c"""
    p = torch.softmax(score, dim=1)
    valid = tgt != 255
    bad = torch.zeros_like(valid)
    for c in range(score.shape[1]):
        e = ((tgt == c).float() - p[:, c]).abs()[valid]
        _, inv, cnt = torch.unique(e, return_inverse=True, return_counts=True)
        t = torch.zeros_like(valid)
        t[valid] = cnt[inv] > 1
        bad |= t
    return bad


def main():
    install_more()
    assert os.path.isdir(REF)
    from mmseg.models.losses.lovasz_loss import LovaszLoss
    from mmseg.models.losses.accuracy import accuracy
    w19 = sibling_class_weight()
    # name, kwargs, (N, C, H, W), share of labels 255, logit scale, the labels drawn (None: every class)
    cases = [
        ('g24_lovasz_default', dict(reduction='none'), (2, 2, 64, 64), 0.1, 3.0, None),
        ('g24_lovasz_all', dict(classes='all', reduction='none'), (2, 2, 64, 64), 0.1, 3.0, None),
        ('g24_lovasz_list1', dict(classes=[1], reduction='none', loss_weight=0.4), (2, 2, 64, 64), 0.1, 3.0, None),
        ('g24_lovasz_cw', dict(class_weight=[0.7, 1.6], reduction='none'), (2, 2, 64, 64), 0.1, 3.0, None),
        ('g24_lovasz_per_image_mean', dict(per_image=True), (2, 2, 64, 64), 0.1, 3.0, None),
        ('g24_lovasz_per_image_sum', dict(per_image=True, reduction='sum', loss_weight=0.4), (2, 2, 48, 40), 0.1, 3.0, None),
        ('g24_lovasz_c5', dict(reduction='none'), (2, 5, 32, 32), 0.1, 2.0, None),
        ('g24_lovasz_c19_few', dict(reduction='none', class_weight=w19), (1, 19, 40, 40), 0.1, 2.0, [0, 3, 7, 11, 18]),
        ('g24_lovasz_c19_all', dict(classes='all', reduction='none'), (1, 19, 40, 40), 0.1, 2.0, [0, 3, 7, 11, 18]),
        ('g24_lovasz_ignore12', dict(reduction='none'), (2, 2, 64, 64), 0.12, 3.0, None),
        # image 1 has no pixel of class 1: 'present' averages one class there, two in image 0
        ('g24_lovasz_no_class1', dict(per_image=True), (2, 2, 64, 64), 0.1, 3.0, 'no_class1'),
    ]
    g = torch.Generator().manual_seed(2400)
    for name, kw, shp, p_ign, scale, draw in cases:
        n, c, h, w = shp
        assert n * h * w <= 8192
        score = scale * torch.randn(shp, generator=g)
        if isinstance(draw, list):
            tgt = torch.tensor(draw)[torch.randint(0, len(draw), (n, h, w), generator=g)]
        else:
            tgt = torch.randint(0, c, (n, h, w), generator=g)
        if draw == 'no_class1':
            tgt[1] = 0
        ign = torch.rand((n, h, w), generator=g) < p_ign
        tgt[ign] = 255
        redrawn = 0
        while True:
            bad = tied_pixels(score, tgt)
            k = int(bad.sum())
            if k == 0:
                break
            redrawn += k
            fresh = scale * torch.randn((k, c), generator=g)
            score.permute(0, 2, 3, 1)[bad] = fresh
        score.requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            crit = LovaszLoss(**kw)
        loss = crit(score, tgt, ignore_index=255)
        loss.backward()
        acc = accuracy(score.detach(), tgt, ignore_index=255)
        print(f'{name}: {redrawn} pixels re-drawn', end='  ')
        save(name, {'score': score.detach(), 'target': tgt}, {'loss': loss.detach(), 'acc': acc}, {'score': score.grad},
             dict(kind='LovaszLoss', kwargs=kw, ignore_index=255))


if __name__ == '__main__':
    main()
