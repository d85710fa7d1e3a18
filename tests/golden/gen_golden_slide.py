#!/usr/bin/env python3
"""Golden vectors for sliding-window inference: the reference's EncoderDecoder.slide_inference
(mmseg/models/segmentors/encoder_decoder.py:241-292), IMPORTED from /root/reference in this container and called
unbound on a stand-in `self`.  Only data is written (tests/golden/g19_slide_*.npz);
re-run: python tests/golden/gen_golden_slide.py

The stand-in carries `test_cfg` (attribute-style dict), `out_channels` and `encode_decode` = a fixed pure function of
the crop: one seeded 3x3 F.conv2d 3 -> C (weights saved in the fixture; accumulated in float64 and rounded once, so
that any machine reproduces the same float32 addends), so the fixture pins the window grid, the
order of the additions and the division by the window count.

Import plumbing: parent packages are empty modules whose __path__ points at the reference directories (no reference
__init__ runs); module-level imports of encoder_decoder.py that the method never executes get NAME-ONLY stand-ins:
mmengine.logging.print_log, mmseg.registry.MODELS.register_module, the type aliases of mmseg.utils, and the base
class of .base (BaseSegmentor = object).
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))


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
    _pkg('mmseg.models.segmentors', f'{REF}/mmseg/models/segmentors')

    class _Reg:
        def register_module(self, *a, **k):
            return lambda cls: cls
    _pkg('mmseg.registry', MODELS=_Reg())
    _pkg('mmseg.utils', **{n: object for n in ('ConfigType', 'OptConfigType', 'OptMultiConfig', 'OptSampleList',
                                               'SampleList', 'add_prefix')})
    _pkg('mmseg.models.segmentors.base', BaseSegmentor=object)
    _pkg('mmengine')
    _pkg('mmengine.logging', print_log=print)


def window_logits(crop_img, w, b):
    """the stand-in network: a 3x3 conv accumulated in float64 and rounded once to float32, so that the addends do not
    depend on which f32 convolution kernel the CPU at hand selects (the test recomputes them on its own machine)"""
    return F.conv2d(crop_img.double(), w.double(), b.double(), padding=1).float()


class AttrDict(dict):
    __getattr__ = dict.__getitem__


CASES = [   # name, N, C, H, W, crop, stride
    ('g19_slide_shift_c19', 1, 19, 37, 53, (16, 24), (9, 11)),       # strides divide neither H - crop nor W - crop
    ('g19_slide_n2_c2', 2, 2, 41, 29, (16, 12), (10, 7)),
    ('g19_slide_bigcrop_h_c19', 1, 19, 20, 53, (32, 24), (16, 13)),  # crop taller than the image
    ('g19_slide_bigcrop_both_c2', 2, 2, 21, 27, (32, 32), (16, 16)), # crop larger in both dimensions: one window
    ('g19_slide_exact_c19', 1, 19, 32, 48, (16, 16), (8, 16)),       # strides divide: no shifted window, W % 4 == 0
]


def main():
    install()
    from mmseg.models.segmentors.encoder_decoder import EncoderDecoder
    for i, (name, N, C, H, W, crop, stride) in enumerate(CASES):
        g = torch.Generator().manual_seed(304 + i)
        x = torch.randn((N, 3, H, W), generator=g)
        w = torch.randn((C, 3, 3, 3), generator=g) * 0.5
        b = torch.randn((C,), generator=g)
        me = types.SimpleNamespace(test_cfg=AttrDict(mode='slide', crop_size=crop, stride=stride), out_channels=C,
                                   encode_decode=lambda crop_img, metas: window_logits(crop_img, w, b))
        metas = [dict(ori_shape=(H, W), img_shape=(H, W)) for _ in range(N)]
        with torch.no_grad():
            out = EncoderDecoder.slide_inference(me, x, metas)        # encoder_decoder.py:241-292
        d = {'in/x': x.numpy(), 'in/w': w.numpy(), 'in/b': b.numpy(), 'out/seg_logits': out.numpy(),
             'meta': np.asarray(json.dumps(dict(kind='slide_inference', mode='slide', crop_size=list(crop),
                                                stride=list(stride), out_channels=C, shim='names only')))}
        np.savez(os.path.join(OUT, name + '.npz'), **d)
        print(name, tuple(out.shape), float(out.abs().max()))


if __name__ == '__main__':
    main()
