#!/usr/bin/env python3
"""Golden vectors for CrossEntropyLoss and DiceLoss: the reference's own classes
(mmseg/models/losses/cross_entropy_loss.py:211-311, dice_loss.py:94-202), IMPORTED from the reference checkout
(gen_golden_class_weight.REF), run on seeded logits and labels.  Only data is written (tests/golden/g22_*.npz: in/score, in/target,
out/loss, out/acc, gin/score, meta with the class name, the constructor kwargs and the call's ignore_index);
re-run: python tests/golden/gen_golden_seg_losses.py

Class weights come without ignored pixels: the reference indexes class_weight[label] before it masks and raises
IndexError on a label of 255 for both values of avg_non_ignore, so that combination has no reference number (the test
checks it against F.cross_entropy(weight=, ignore_index=255, reduction='mean')).  The 19-class weight list is read at
generation time from the sibling config of the LED-Net one, as gen_golden_class_weight.py does.

Import plumbing (as gen_golden_class_weight.py): parent packages are empty modules whose __path__ points at the
reference directories; NAME-ONLY stand-ins for mmseg.registry.MODELS.register_module and for mmengine.fileio.load,
which losses/utils.py imports (never called: no class_weight is a file path here).
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_class_weight import REF, _pkg, install, sibling_class_weight  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def install_all():
    install()

    def load(*a, **k):
        raise RuntimeError('mmengine.fileio.load: stand-in, not callable')
    _pkg('mmengine')
    _pkg('mmengine.fileio', load=load)


def save(name, inputs, outputs, gin, meta):
    d = {}
    for k, v in inputs.items():
        d['in/' + k] = v.detach().numpy()
    for k, v in outputs.items():
        d['out/' + k] = v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)
    for k, v in gin.items():
        d['gin/' + k] = v.detach().numpy()
    d['meta'] = np.asarray(json.dumps(meta))
    path = os.path.join(OUT, name + '.npz')
    np.savez(path, **d)
    print(f'{name}: {os.path.getsize(path) / 1024:.0f} KiB  loss {float(outputs["loss"]):.6f}')


def main():
    install_all()
    assert os.path.isdir(REF)
    from mmseg.models.losses.cross_entropy_loss import CrossEntropyLoss
    from mmseg.models.losses.dice_loss import DiceLoss
    from mmseg.models.losses.accuracy import accuracy
    w19 = sibling_class_weight()
    kinds = {'DiceLoss': DiceLoss, 'CrossEntropyLoss': CrossEntropyLoss}
    # name, class, kwargs, ignore_index of the call, (N, C, H, W), share of labels 255, logit scale
    cases = [
        ('g22_dice_sigmoid', 'DiceLoss', dict(), 255, (2, 2, 64, 64), 0.1, 3.0),
        ('g22_dice_softmax', 'DiceLoss', dict(use_sigmoid=False), 255, (2, 2, 64, 64), 0.1, 3.0),
        ('g22_dice_naive', 'DiceLoss', dict(naive_dice=True), 255, (2, 2, 64, 64), 0.1, 3.0),
        ('g22_dice_sum_w3', 'DiceLoss', dict(reduction='sum', loss_weight=3.0, eps=1.0), 255, (2, 2, 64, 64), 0.1, 3.0),
        ('g22_dice_skip_class0', 'DiceLoss', dict(ignore_index=0), 255, (2, 2, 64, 64), 0.1, 3.0),
        ('g22_dice_c5_softmax', 'DiceLoss', dict(use_sigmoid=False), 255, (2, 5, 32, 32), 0.1, 2.0),
        ('g22_dice_all_ignored', 'DiceLoss', dict(), 255, (1, 2, 16, 16), 1.0, 1.0),
        ('g22_ce_plain', 'CrossEntropyLoss', dict(), 255, (2, 2, 64, 64), 0.0, 3.0),
        ('g22_ce_ignore_avg_all', 'CrossEntropyLoss', dict(avg_non_ignore=False), 255, (2, 2, 64, 64), 0.2, 3.0),
        ('g22_ce_ignore_avg_valid', 'CrossEntropyLoss', dict(avg_non_ignore=True), 255, (2, 2, 64, 64), 0.2, 3.0),
        ('g22_ce_sum', 'CrossEntropyLoss', dict(reduction='sum', loss_weight=0.4), 255, (2, 2, 48, 40), 0.2, 3.0),
        ('g22_ce_cw', 'CrossEntropyLoss', dict(class_weight=[0.7, 1.6], avg_non_ignore=True), 255, (2, 2, 64, 64), 0.0, 3.0),
        ('g22_ce_c19_cw', 'CrossEntropyLoss', dict(class_weight=w19, loss_weight=0.4), 255, (1, 19, 40, 40), 0.0, 2.0),
    ]
    g = torch.Generator().manual_seed(2200)
    for name, kind, kw, ign_idx, shp, p_ign, scale in cases:
        n, c, h, w = shp
        score = (scale * torch.randn(shp, generator=g)).requires_grad_(True)
        tgt = torch.randint(0, c, (n, h, w), generator=g)
        ign = torch.rand((n, h, w), generator=g) < p_ign
        tgt[ign] = 255
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            crit = kinds[kind](**kw)
        loss = crit(score, tgt, ignore_index=ign_idx)
        loss.backward()
        acc = accuracy(score.detach(), tgt, ignore_index=255)
        save(name, {'score': score.detach(), 'target': tgt}, {'loss': loss.detach(), 'acc': acc}, {'score': score.grad},
             dict(kind=kind, kwargs=kw, ignore_index=ign_idx))


if __name__ == '__main__':
    main()
