#!/usr/bin/env python3
"""Golden vectors for OhemCrossEntropy with class_weight: the reference's own class
(mmseg/models/losses/ohem_cross_entropy_loss.py:11-94), IMPORTED from /root/reference in this container, run on
seeded logits and labels.  Only data is written (tests/golden/g21_ohemcw_*.npz: in/score, in/target, out/loss,
out/acc, gin/score, meta with the constructor kwargs, class_weight included);
re-run: python tests/golden/gen_golden_class_weight.py

The prefix is g21_ohemcw_, not g7_: the g7_ fixtures are the unweighted ones (another test feeds every g7_* file to the
unweighted specification).  The 19-class weight list is read at generation time from the sibling config of the
LED-Net one (configs/LED_Net/ddrnet_23_in1k-pre_2xb6-120k_cityscapes-1024x1024.py:14-18, the list both of its
OhemCrossEntropy losses use) and travels only as the fixture's meta.

Import plumbing: parent packages are empty modules whose __path__ points at the reference directories; a NAME-ONLY
stand-in for mmseg.registry.MODELS.register_module, the one name ohem_cross_entropy_loss.py imports from mmseg.
losses/accuracy.py (accuracy, for out/acc) imports torch only.
"""
import ast
import json
import os
import re
import sys
import types

import numpy as np
import torch

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))
SIBLING_CFG = f'{REF}/configs/LED_Net/ddrnet_23_in1k-pre_2xb6-120k_cityscapes-1024x1024.py'


def _pkg(name, path=None, **names):
    m = types.ModuleType(name)
    m.__path__ = [path] if path else []
    for k, v in names.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def install():
    _pkg('mmseg', f'{REF}/mmseg')
    _pkg('mmseg.models', f'{REF}/mmseg/models')
    _pkg('mmseg.models.losses', f'{REF}/mmseg/models/losses')

    class _Reg:
        def register_module(self, *a, **k):
            return lambda cls: cls
    _pkg('mmseg.registry', MODELS=_Reg())


def sibling_class_weight():
    """the `class_weight = [...]` literal of the sibling config (a list of 19 floats)"""
    src = open(SIBLING_CFG).read()
    m = re.search(r'^class_weight = (\[.*?\])', src, flags=re.M | re.S)
    w = ast.literal_eval(m.group(1))
    assert len(w) == 19 and all(isinstance(v, float) for v in w)
    return w


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
    install()
    from mmseg.models.losses.ohem_cross_entropy_loss import OhemCrossEntropy
    from mmseg.models.losses.accuracy import accuracy
    w19 = sibling_class_weight()
    # name, kwargs, (N, C, H, W), share of ignored pixels, logit scale
    cases = [
        # two classes, 64 x 64, 10 % ignored: min_kept below / above the valid count
        ('g21_ohemcw_k1000', dict(thres=0.9, min_kept=1000, loss_weight=1.0, class_weight=[0.7, 1.6]), (2, 2, 64, 64), 0.1, 3.0),
        ('g21_ohemcw_k131072', dict(thres=0.9, min_kept=131072, loss_weight=0.4, class_weight=[0.7, 1.6]), (2, 2, 64, 64), 0.1, 3.0),
        # confident logits: the k-th probability is above thres only for few pixels -- thres decides
        ('g21_ohemcw_k100_confident', dict(thres=0.7, min_kept=100, loss_weight=1.0, class_weight=[0.7, 1.6]), (1, 2, 48, 40), 0.0, 8.0),
        ('g21_ohemcw_c5', dict(thres=0.9, min_kept=500, loss_weight=1.0, class_weight=[0.5, 2.0, 1.0, 1.25, 0.8]), (2, 5, 32, 32), 0.2, 2.0),
        ('g21_ohemcw_c19', dict(thres=0.9, min_kept=600, loss_weight=0.4, class_weight=w19), (1, 19, 40, 40), 0.1, 2.0),
        # a zero weight: "divide by the count" and "divide by the sum of the weights" give different losses
        ('g21_ohemcw_zero_one', dict(thres=0.9, min_kept=1000, loss_weight=1.0, class_weight=[0.0, 1.0]), (2, 2, 64, 64), 0.1, 3.0),
        ('g21_ohemcw_all_ignored', dict(thres=0.9, min_kept=1000, loss_weight=1.0, class_weight=[0.7, 1.6]), (1, 2, 16, 16), 1.0, 1.0),
    ]
    g = torch.Generator().manual_seed(2100)
    for name, kw, shp, p_ign, scale in cases:
        n, c, h, w = shp
        score = (scale * torch.randn(shp, generator=g)).requires_grad_(True)
        tgt = torch.randint(0, c, (n, h, w), generator=g)
        ign = torch.rand((n, h, w), generator=g) < p_ign
        tgt[ign] = 255
        crit = OhemCrossEntropy(**kw)
        loss = crit(score, tgt)
        gin = {}
        if loss.requires_grad:
            loss.backward()
            gin = {'score': score.grad}
        acc = accuracy(score.detach(), tgt, ignore_index=255)
        save(name, {'score': score.detach(), 'target': tgt}, {'loss': loss.detach(), 'acc': acc}, gin,
             dict(kind='OhemCrossEntropy', kwargs=kw))


if __name__ == '__main__':
    main()
