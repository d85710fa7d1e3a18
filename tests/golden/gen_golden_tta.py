#!/usr/bin/env python3
"""Golden vectors for the test-time-augmentation merge: the reference's SegTTAModel.merge_preds
(mmseg/models/segmentors/seg_tta.py:15-47), IMPORTED from /root/reference in this container and called unbound on a
stand-in `self` (self.module.out_channels).  Only data is written (tests/golden/g20_tta_merge_*.npz);
re-run: python tests/golden/gen_golden_tta.py

The method returns only the mask, so the expected mean probabilities are recomputed here with the method's own
statements (zeros; += softmax(dim=0) view by view; /= K) and checked to reproduce the method's mask exactly.  Per
fixture the share of pixels whose top-two merged probabilities differ by less than 1e-5 (near ties, where two correct
f32 implementations may pick different classes) is recorded, and a fixture with more than 1 % of them is refused.

Import plumbing: parent packages are empty modules whose __path__ points at the reference directories; NAME-ONLY
stand-ins for what seg_tta.py imports at module level: mmengine.model.BaseTTAModel (= object),
mmengine.structures.PixelData (a one-field holder: merge_preds wraps the mask in it), mmseg.registry.MODELS
.register_module, mmseg.utils.SampleList.  The samples are plain holders with the two setters the method calls.
"""
import json
import os
import sys
import types

import numpy as np
import torch

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))
TIE, TIE_CAP = 1e-5, 0.01


def _pkg(name, path=None, **names):
    m = types.ModuleType(name)
    m.__path__ = [path] if path else []
    for k, v in names.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


class PixelData:
    def __init__(self, data=None):
        self.data = data


class Sample:
    def __init__(self, logits, img_path):
        self.seg_logits = PixelData(logits)
        self.img_path = img_path

    def set_data(self, d):
        for k, v in d.items():
            setattr(self, k, v)

    def set_metainfo(self, d):
        for k, v in d.items():
            setattr(self, k, v)


def install():
    _pkg('mmseg', f'{REF}/mmseg')
    _pkg('mmseg.models', f'{REF}/mmseg/models')
    _pkg('mmseg.models.segmentors', f'{REF}/mmseg/models/segmentors')

    class _Reg:
        def register_module(self, *a, **k):
            return lambda cls: cls
    _pkg('mmseg.registry', MODELS=_Reg())
    _pkg('mmseg.utils', SampleList=object)
    _pkg('mmengine')
    _pkg('mmengine.model', BaseTTAModel=object)
    _pkg('mmengine.structures', PixelData=PixelData)


CASES = [   # name, K, C, H, W, logit scale
    ('g20_tta_merge_k12_c19', 12, 19, 23, 29, 3.0),        # (12 x 19 planes: a larger image would pass the 1 MiB file cap)
    ('g20_tta_merge_k2_c19', 2, 19, 41, 28, 3.0),
    ('g20_tta_merge_k1_c19', 1, 19, 16, 24, 3.0),
    ('g20_tta_merge_k12_c2', 12, 2, 37, 53, 3.0),
    ('g20_tta_merge_k2_c2', 2, 2, 33, 31, 3.0),
    ('g20_tta_merge_k1_c2', 1, 2, 24, 36, 3.0),
]


def main():
    install()
    from mmseg.models.segmentors.seg_tta import SegTTAModel
    for i, (name, K, C, H, W, scale) in enumerate(CASES):
        g = torch.Generator().manual_seed(304 + i)
        views = scale * torch.randn((K, C, H, W), generator=g)
        me = types.SimpleNamespace(module=types.SimpleNamespace(out_channels=C))
        samples = [Sample(views[k].clone(), 'img.png') for k in range(K)]
        merged = SegTTAModel.merge_preds(me, [samples])               # seg_tta.py:15-47
        mask = merged[0].pred_sem_seg.data
        probs = torch.zeros(views[0].shape).to(views[0])              # the method's own statements (:28-35)
        for k in range(K):
            probs += views[k].softmax(dim=0)
        probs /= K
        assert torch.equal(probs.argmax(dim=0), mask), 'the restated mean does not reproduce the method\'s mask'
        top2 = probs.topk(2, dim=0).values
        share = float(((top2[0] - top2[1]) < TIE).float().mean())
        if share > TIE_CAP:
            raise SystemExit(f'{name}: {share:.2%} of the pixels are near ties (< {TIE}): lower the logit scale')
        d = {'in/views': views.numpy(), 'out/probs': probs.numpy(), 'out/mask': mask.numpy().astype(np.uint8),
             'meta': np.asarray(json.dumps(dict(kind='SegTTAModel.merge_preds', K=K, out_channels=C, logit_scale=scale,
                                                tie_band=TIE, tie_share=share, shim='names only')))}
        np.savez(os.path.join(OUT, name + '.npz'), **d)
        print(name, f'near-tie share {share:.4%}')


if __name__ == '__main__':
    main()
