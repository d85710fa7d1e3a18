"""Sliding-window inference and multi-scale / flip test-time augmentation with the fused merge kernels
(csrc/tta_merge.hip: ledn_tta_accumulate, ledn_slide_accumulate, ledn_slide_finish) -- against the reference's
EncoderDecoder.slide_inference and SegTTAModel.merge_preds (fixtures g19 / g20, tests/golden/gen_golden_slide.py,
gen_golden_tta.py) and torch compositions on the CPU.  Kernel tests run on the emulator and, under -m gpu, on the
HIP build through the same C ABI.

Tolerances.  PROB_TOL: the merged probabilities against the reference's CPU f32 softmax; measured maximum absolute
difference on the g20 fixtures: emulator 1.192e-7, HIP build (MI355X) 1.192e-7 (EXPERIMENTS.md) -> twice the larger.  Masks are
compared on every pixel whose golden top-two gap is >= TIE; the excluded share is capped at 1 %."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, golden_names, slow_on_emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_test_config.py')
PROB_TOL = 2 * 1.192e-7
TIE, TIE_CAP = 1e-5, 0.01
RATIOS = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]


def _npz(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    return {k: (json.loads(str(z[k])) if k == 'meta' else torch.from_numpy(np.array(z[k]))) for k in z.files}


def _model(be, test_cfg=None, seed=21):
    import led_net_amd as L
    torch.manual_seed(seed)
    cfg = L.load_config(CFG)
    mcfg = dict(cfg['model'])
    if test_cfg is not None:
        mcfg['test_cfg'] = test_cfg
    return L, L.MODELS.build(mcfg).to(be.dev).eval()


def _check_mask(mask, probs, label=''):
    """mask == argmax wherever the golden top-two gap is >= TIE; the near-tie share stays under the cap"""
    top2 = probs.topk(2, dim=0).values
    clear = (top2[0] - top2[1]) >= TIE
    share = 1.0 - clear.float().mean().item()
    print(f'{label} near-tie share {share:.4%}')
    assert share <= TIE_CAP
    assert ((mask.long() != probs.argmax(0)) & clear).sum().item() == 0


# ---- 1. slide_inference against the reference's, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize('name', golden_names('g19_slide_'))
def test_slide_inference_equals_the_reference_bit_for_bit(be, name):
    fx = _npz(name)
    meta = fx['meta']
    L, model = _model(be, dict(mode='slide', crop_size=tuple(meta['crop_size']), stride=tuple(meta['stride'])))
    model.out_channels = meta['out_channels']
    w, b = fx['in/w'], fx['in/b']
    # the fixture's conv runs on the CPU exactly as the generator ran it (accumulated in float64, rounded once: the same
    # float32 addends on any machine) and its output is handed to the backend: the kernels under test face the golden
    # bit for bit on the emulator AND on the HIP build
    model.encode_decode = lambda crop, metas=None: be(F.conv2d(crop.cpu().double(), w.double(), b.double(), padding=1).float())
    x = be(fx['in/x'])
    with torch.no_grad():
        logits, mask = model.slide_inference(x, [dict(ori_shape=tuple(x.shape[2:])) for _ in range(x.shape[0])],
                                             return_mask=True)
    want = fx['out/seg_logits']
    print(f'{name} [{be.dev.type}]: max |diff| vs the reference = {(logits.cpu() - want).abs().max().item():.3e}')
    assert torch.equal(logits.cpu(), want)
    assert torch.equal(mask.cpu().long(), want.argmax(1))


def test_slide_grid_is_the_reference_grid(be):
    L, model = _model(be, dict(mode='slide', crop_size=(16, 24), stride=(9, 11)))
    boxes, rowcnt, colcnt = model.slide_grid(37, 53)
    assert boxes[0] == (0, 16, 0, 24) and boxes[-1] == (21, 37, 29, 53) and len(boxes) == 4 * 4
    count = torch.zeros(37, 53, dtype=torch.int32)
    for y1, y2, x1, x2 in boxes:
        count[y1:y2, x1:x2] += 1
    assert torch.equal(count, rowcnt[:, None] * colcnt[None, :]) and int(count.min()) >= 1
    assert model.slide_grid(10, 12)[0] == [(0, 10, 0, 12)]        # crop larger than the image: the small patch


# ---- 2. whole tiny network ----------------------------------------------------------------------------------------------
def test_slide_with_one_window_equals_whole(be):
    L, whole = _model(be)
    _, slide = _model(be, dict(mode='slide', crop_size=(320, 384), stride=(64, 64)))
    x = be(torch.randn(1, 3, 288, 320, generator=torch.Generator().manual_seed(5)))
    assert slide.slide_grid(288, 320)[0] == [(0, 288, 0, 320)]
    from led_net_amd import ops
    launched = []
    run = ops._run
    ops._run = lambda lib, name, *a, **k: (launched.append(name), run(lib, name, *a, **k))[1]
    try:
        with torch.no_grad():
            a, b = whole(x, None, mode='predict'), slide(x, None, mode='predict')
    finally:
        ops._run = run
    assert launched.count('ledn_slide_accumulate') == 1 and launched.count('ledn_slide_finish') == 1
    for da, db in zip(a, b):
        assert torch.equal(da.seg_logits.data, db.seg_logits.data)
        assert torch.equal(da.pred_sem_seg.data, db.pred_sem_seg.data) and db.pred_sem_seg.data.dtype == torch.uint8


def test_slide_grid_equals_the_composition_of_window_predictions(be):
    slow_on_emu(be.dev)                  # 12 forwards of the network (its GETB stage needs inputs of 257 pixels and more)
    L, whole = _model(be)
    _, slide = _model(be, dict(mode='slide', crop_size=(288, 320), stride=(64, 96)))
    x = be(torch.randn(1, 3, 352, 500, generator=torch.Generator().manual_seed(6)))
    boxes = slide.slide_grid(352, 500)[0]
    assert len(boxes) == 2 * 3
    with torch.no_grad():
        got = slide(x, None, mode='predict')[0]
        canvas = torch.zeros_like(got.seg_logits.data)[None]
        count = torch.zeros((1, 1, 352, 500), device=x.device)
        for y1, y2, x1, x2 in boxes:
            lg = whole(x[:, :, y1:y2, x1:x2].contiguous(), None, mode='predict')[0].seg_logits.data[None]
            canvas += F.pad(lg, (x1, 500 - x2, y1, 352 - y2))
            count[:, :, y1:y2, x1:x2] += 1
    want = (canvas / count)[0]
    assert torch.equal(got.seg_logits.data, want)
    assert torch.equal(got.pred_sem_seg.data.long(), want.argmax(0, keepdim=True))


@pytest.mark.parametrize('N,C,H,W,box', [(2, 19, 24, 32, (4, 20, 8, 28)), (2, 19, 21, 30, (3, 19, 5, 27)),
                                         (2, 2, 24, 32, (0, 24, 12, 32)), (2, 2, 17, 23, (1, 16, 2, 21)),
                                         (1, 8, 16, 16, (8, 16, 4, 12))])
def test_slide_accumulate_both_crop_layouts(be, N, C, H, W, box):
    """canvas[:, :, y1:y2, x1:x2] += crop for NHWC and planar crops, 16-byte (W, x1, wc multiples of 4) and scalar paths"""
    from led_net_amd import ops
    y1, y2, x1, x2 = box
    g = torch.Generator().manual_seed(C * H + W)
    base = torch.randn((N, C, H, W), generator=g)
    crop = torch.randn((N, C, y2 - y1, x2 - x1), generator=g)
    want = base.clone()
    want[:, :, y1:y2, x1:x2] += crop
    for planar in (False, True):
        canvas = be(base.clone())
        ops.slide_accumulate(canvas, be(crop.contiguous() if planar else crop.permute(0, 2, 3, 1).contiguous()), y1, x1,
                             planar=planar)
        assert torch.equal(canvas.cpu(), want), f'planar={planar}'
    rowcnt = torch.randint(1, 4, (H,), generator=g).int()
    colcnt = torch.randint(1, 4, (W,), generator=g).int()
    mask = ops.slide_finish(canvas, rowcnt, colcnt)
    div = want / (rowcnt[:, None] * colcnt[None, :]).float()
    assert torch.equal(canvas.cpu(), div) and torch.equal(mask.cpu().long(), div.argmax(1))


def test_slide_mode_on_padded_and_flipped_samples(be):
    """slide mode behind the data preprocessor's batch padding, with a flipped and a resized sample: windows that hold
    padding get it from the stem's input kernel like a padded whole image, and the finished canvas goes through
    postprocess_result -- equal to the same windows composed by hand from whole-mode forwards of the padded crops"""
    slow_on_emu(be.dev)
    L, whole = _model(be)
    _, slide = _model(be, dict(mode='slide', crop_size=(288, 288), stride=(96, 96)))
    for m in (whole, slide):
        m.data_preprocessor.test_cfg = dict(size_divisor=64)
    g = torch.Generator().manual_seed(12)
    imgs = [torch.randint(0, 256, (3, 300, 330), dtype=torch.uint8, generator=g) for _ in range(2)]

    def samples():
        return [L.SegDataSample(metainfo=dict(ori_shape=(300, 330), flip=True, flip_direction='horizontal')),
                L.SegDataSample(metainfo=dict(ori_shape=(210, 225)))]
    data = slide.data_preprocessor(dict(inputs=imgs, data_samples=samples()), training=False)
    x = data['inputs']
    assert tuple(x.shape) == (2, 3, 320, 384) and data['data_samples'][0].metainfo['img_padding_size'] == (0, 54, 0, 20)
    boxes = slide.slide_grid(320, 384)[0]
    assert len(boxes) == 2 * 2
    with torch.no_grad():
        got = slide(x, data['data_samples'], mode='predict')
        canvas = torch.zeros((2, 2, 320, 384), device=x.device)
        count = torch.zeros((1, 1, 320, 384), device=x.device)
        for y1, y2, x1, x2 in boxes:
            pad = (0, max(x2 - 330, 0), 0, max(y2 - 300, 0))
            ws = [L.SegDataSample(metainfo=dict(img_padding_size=pad)) for _ in range(2)]
            lg = whole.decode_head.predict(whole.extract_feat(x[:, :, y1:y2, x1:x2].contiguous(), ws))
            canvas += F.pad(lg, (x1, 384 - x2, y1, 320 - y2))
            count[:, :, y1:y2, x1:x2] += 1
        padded = slide.data_preprocessor(dict(inputs=imgs, data_samples=samples()), training=False)['data_samples']
        want = whole.postprocess_result((canvas / count).permute(0, 2, 3, 1).contiguous(), padded)
    for a, b in zip(got, want):
        assert tuple(a.seg_logits.data.shape) == (2,) + tuple(a.metainfo['ori_shape'])
        assert torch.equal(a.seg_logits.data, b.seg_logits.data) and torch.equal(a.pred_sem_seg.data, b.pred_sem_seg.data)
    # the TTA model over a slide-mode module: planar logits of `inference` into the accumulator
    view = dict(inputs=[imgs], data_samples=[samples()])
    out = L.SegTTAModel(module=slide).test_step(view)
    for i, ds in enumerate(out):
        ref = want[i].seg_logits.data.cpu().softmax(0)
        err = (ds.seg_logits.data.cpu() - ref).abs().max().item()
        print(f'slide-mode TTA, one view, image {i} [{be.dev.type}]: max |prob - softmax(slide predict)| = {err:.3e}')
        assert err <= PROB_TOL
        _check_mask(ds.pred_sem_seg.data.cpu()[0], ref, f'slide tta {i}')


# ---- 3. a test_cfg that cannot be honoured is an error ------------------------------------------------------------------
def test_unknown_mode_and_incomplete_slide_cfg_raise(be):
    x = be(torch.randn(1, 3, 64, 64))
    _, model = _model(be, dict(mode='bogus'))
    with pytest.raises(AssertionError, match='Only "slide" or "whole" test mode are supported'):
        model(x, None, mode='predict')
    with pytest.raises(AssertionError, match='Only "slide" or "whole"'):
        model.inference(x, None)
    for cfg in (dict(mode='slide'), dict(mode='slide', crop_size=(32, 32)), dict(mode='slide', stride=(16, 16)),
                dict(mode='slide', crop_size=(32, 32), stride=(0, 16))):
        _, model = _model(be, cfg)
        with pytest.raises(ValueError, match="mode='slide' needs (crop_size|stride)"):
            model(x, None, mode='predict')


# ---- 4. merge_preds against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', golden_names('g20_tta_merge_'))
def test_merge_preds_equals_the_reference(be, name):
    fx = _npz(name)
    L, model = _model(be)
    model.out_channels = fx['meta']['out_channels']
    tta = L.SegTTAModel(module=model)
    gt = torch.zeros(1, 4, 4)
    samples = []
    for k, v in enumerate(fx['in/views']):
        ds = L.SegDataSample(gt=gt if k == 0 else None, metainfo=dict(img_path=f'view{k}.png'))
        ds.seg_logits = L.segmentor.PixelData(data=be(v.contiguous()))
        samples.append(ds)
    merged = tta.merge_preds([samples])
    assert len(merged) == 1 and merged[0] is samples[-1]
    probs, mask = merged[0].seg_logits.data.cpu(), merged[0].pred_sem_seg.data.cpu()
    err = (probs - fx['out/probs']).abs().max().item()
    print(f'{name} [{be.dev.type}]: max |prob - golden| = {err:.3e}')
    assert err <= PROB_TOL
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (1,) + tuple(probs.shape[1:])
    _check_mask(mask[0], fx['out/probs'], name)
    if fx['meta']['tie_share'] == 0.0:
        assert torch.equal(mask[0], fx['out/mask'])
    assert merged[0].gt_sem_seg.data is gt and merged[0].metainfo['img_path'] == 'view0.png'


# ---- 5. tta_accumulate with real geometry ---------------------------------------------------------------------------------
GEOMETRY = [   # C, (Ho, Wo), [per view: ratio, (pad_bottom, pad_right), flip, planar]
    (19, (37, 53), [(0.5, (0, 0), None, False), (0.75, (3, 5), 'horizontal', False), (1.25, (0, 7), 'vertical', True),
                    (1.75, (2, 0), 'horizontal', True)]),
    (19, (24, 52), [(1.25, (1, 3), 'horizontal', False), (1.0, (0, 0), None, False), (0.5, (0, 0), 'vertical', False)]),
    (2, (41, 28), [(1.75, (0, 0), 'vertical', False), (0.5, (4, 4), None, True)]),
    (2, (33, 31), [(0.75, (0, 1), 'horizontal', True)]),
    (5, (20, 24), [(1.5, (2, 2), 'horizontal', False), (1.0, (0, 0), 'horizontal', True)]),
]


@pytest.mark.parametrize('mode', ['softmax', 'raw'])
@pytest.mark.parametrize('case', range(len(GEOMETRY)))
def test_tta_accumulate_geometry(be, case, mode):
    """crop -> flip -> F.interpolate(bilinear, align_corners=False) -> softmax -> sum -> / K in torch f32 on the CPU;
    unit-scale randn logits.  Softmax mode: PROB_TOL.  Raw mode: both sides round the source coordinate once, what is
    left is the order and fusing of the lerp's products and sums: two f32 spacings of a logit (|logit| < 8: 4.77e-7
    each) -> 9.5e-7.  Measured: emulator and HIP build (MI355X) at most 1.2e-7 (softmax) and 2.4e-7 (raw)."""
    from led_net_amd import ops
    C, (Ho, Wo), views = GEOMETRY[case]
    g = torch.Generator().manual_seed(100 + case)
    K = len(views)
    acc = torch.empty((C, Ho, Wo), device=be.dev)
    mask = torch.empty((Ho, Wo), dtype=torch.uint8, device=be.dev)
    want = torch.zeros(C, Ho, Wo)
    for k, (ratio, (pb, pr), flip, planar) in enumerate(views):
        hv, wv = int(Ho * ratio + 0.5), int(Wo * ratio + 0.5)
        src = torch.randn((C, hv + pb, wv + pr), generator=g)
        v = src[None, :, :hv, :wv]
        if flip:
            v = v.flip(dims=(3,) if flip == 'horizontal' else (2,))
        v = F.interpolate(v, size=(Ho, Wo), mode='bilinear', align_corners=False)[0]
        want += v.softmax(0) if mode == 'softmax' else v
        s = be(src.contiguous() if planar else src.permute(1, 2, 0).contiguous())
        ops.tta_accumulate(s, acc, first=k == 0, last=k == K - 1, K=K, valid=(hv, wv), flip=flip, planar=planar,
                           mode=mode, mask=mask if k == K - 1 else None)
    want /= K
    err = (acc.cpu() - want).abs().max().item()
    print(f'geometry case {case} {mode} [{be.dev.type}]: max |diff| = {err:.3e}')
    assert err <= (PROB_TOL if mode == 'softmax' else 2 * 4.77e-7)
    _check_mask(mask.cpu(), want, f'case {case} {mode}')


@pytest.mark.parametrize('C,src_hw,out_hw', [(19, (20, 27), (37, 52)), (19, (45, 61), (37, 53)), (2, (33, 31), (33, 31)),
                                             (8, (12, 10), (21, 16))])
def test_tta_raw_single_view_is_the_bilinear_kernel(be, C, src_hw, out_hw):
    from led_net_amd import ops
    x = be(torch.randn((1,) + src_hw + (C,), generator=torch.Generator().manual_seed(C)))
    y, am = ops.bilinear(x, out_hw, nchw=True, argmax=True)
    acc = torch.empty((C,) + out_hw, device=be.dev)
    mask = torch.empty(out_hw, dtype=torch.uint8, device=be.dev)
    ops.tta_accumulate(x[0], acc, first=True, last=True, K=1, mode='raw', mask=mask)
    diff = (acc - y[0]).abs().max().item()
    ulp = 2.0 ** (np.floor(np.log2(x.abs().max().item())) - 23)          # f32 spacing at the largest logit
    print(f'raw single view vs ops.bilinear [{be.dev.type}] C{C} {src_hw}->{out_hw}: max |diff| = {diff:.3e} (ulp {ulp:.3e})')
    if be.dev.type == 'cpu':
        assert torch.equal(acc, y[0]) and torch.equal(mask, am[0])
    else:
        # the device compiler contracts the lerp into fused multiply-adds differently in the two kernels (measured on
        # the MI355X: at most 1 ulp of the logit, EXPERIMENTS.md); the mask is the first-max argmax of what was written
        assert diff <= ulp
        assert torch.equal(mask.long(), acc.argmax(0))


def test_tta_first_overwrites_and_middle_views_do_not_divide(be):
    from led_net_amd import ops
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn((19, 10, 12), generator=g), torch.randn((19, 10, 12), generator=g)
    acc = be(torch.full((19, 10, 12), float('nan')))
    ops.tta_accumulate(be(a), acc, first=True, last=False, K=2, planar=True, mode='raw')
    assert torch.equal(acc.cpu(), a)
    ops.tta_accumulate(be(b), acc, first=False, last=False, K=2, planar=True, mode='raw')
    assert torch.equal(acc.cpu(), a + b)


# ---- 6. / 7. TestTimeAug and SegTTAModel.test_step on the tiny network ----------------------------------------------------
def _tta(L):
    return L.transforms.TestTimeAug(transforms=[
        [dict(type='Resize', scale_factor=r, keep_ratio=True) for r in RATIOS],
        [dict(type='RandomFlip', prob=0., direction='horizontal'), dict(type='RandomFlip', prob=1., direction='horizontal')],
        [dict(type='LoadAnnotations')], [dict(type='PackSegInputs')]])


def test_test_time_aug_views(be):
    import led_net_amd as L
    tta = _tta(L)
    assert len(tta) == 12
    g = torch.Generator().manual_seed(3)
    img = be(torch.randint(0, 256, (45, 62, 3), dtype=torch.uint8, generator=g))
    gt = be(torch.randint(0, 2, (45, 62), dtype=torch.uint8, generator=g))
    out = tta.transform(dict(img=img, gt_seg_map=gt, img_path='a.png'))
    assert set(out) == {'inputs', 'data_samples'} and len(out['inputs']) == len(out['data_samples']) == 12
    for k, (inp, ds) in enumerate(zip(out['inputs'], out['data_samples'])):
        r, flip = RATIOS[k // 2], bool(k % 2)                       # scale-major, flip-minor
        w, h = int(int(62 * r + 0.5)), int(int(45 * r + 0.5))
        m = ds.metainfo
        assert tuple(inp.shape) == (3, m['img_shape'][0], m['img_shape'][1]) and inp.dtype == torch.uint8
        assert abs(m['img_shape'][0] - h) <= 1 and abs(m['img_shape'][1] - w) <= 1
        assert m['scale_factor'] == (m['img_shape'][1] / 62, m['img_shape'][0] / 45)
        assert m['ori_shape'] == (45, 62) and m['flip'] is flip and m['img_path'] == 'a.png'
        assert m['flip_direction'] == ('horizontal' if flip else None)
        assert torch.equal(ds.gt_sem_seg.data, gt[None].long())      # the label map stays at the original size
    for k in (4, 5):                                                  # ratio 1.0: the image itself / its mirror
        want = img.permute(2, 0, 1)
        assert torch.equal(out['inputs'][k], want.flip(dims=(2,)) if k % 2 else want)
    data = L.transforms.collate_views([out, out])
    assert len(data['inputs']) == 12 and len(data['inputs'][0]) == 2 and data['data_samples'][3][1] is out['data_samples'][3]


def test_tta_test_step_equals_predict_per_view_then_merge(be):
    slow_on_emu(be.dev)
    import copy
    import led_net_amd as L
    _, model = _model(be)
    model.data_preprocessor.test_cfg = dict(size_divisor=32)        # views are padded: the merge has to un-pad them
    tta_model = L.MODELS.build(dict(type='SegTTAModel', module=model))
    g = torch.Generator().manual_seed(4)
    packed = []
    for _ in range(2):
        img = be(torch.randint(0, 256, (530, 600, 3), dtype=torch.uint8, generator=g))     # (0.5 x: 265 x 300, the
        gt = be(torch.randint(0, 2, (530, 600), dtype=torch.uint8, generator=g))            # smallest the network takes)
        packed.append(_tta(L).transform(dict(img=img, gt_seg_map=gt)))
    data = L.transforms.collate_views(packed)
    slow_views = []
    with torch.no_grad():
        for k in range(12):
            d = model.data_preprocessor(dict(inputs=data['inputs'][k], data_samples=copy.deepcopy(data['data_samples'][k])), False)
            slow_views.append(model(d['inputs'], d['data_samples'], mode='predict'))
    slow = tta_model.merge_preds([[slow_views[k][i] for k in range(12)] for i in range(2)])
    fast = tta_model.test_step(data)
    assert len(fast) == 2
    for i in range(2):
        a, b = fast[i].seg_logits.data.cpu(), slow[i].seg_logits.data.cpu()
        assert tuple(a.shape) == (2, 530, 600)
        err = (a - b).abs().max().item()
        print(f'test_step vs predict + merge_preds, image {i} [{be.dev.type}]: max |diff| = {err:.3e}')
        assert err <= PROB_TOL
        _check_mask(fast[i].pred_sem_seg.data.cpu()[0], b, f'image {i}')
        assert torch.equal(fast[i].gt_sem_seg.data, data['data_samples'][0][i].gt_sem_seg.data)


def test_tta_single_view_is_the_softmax_of_predict(be):
    import led_net_amd as L
    _, model = _model(be)
    tta = L.transforms.TestTimeAug(transforms=[[dict(type='Resize', scale_factor=1.0, keep_ratio=True)],
                                                [dict(type='RandomFlip', prob=0.)], [dict(type='PackSegInputs')]])
    img = be(torch.randint(0, 256, (288, 324, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(8)))
    out = L.SegTTAModel(module=model).test_step(L.transforms.collate_views([tta.transform(dict(img=img))]))
    with torch.no_grad():
        ref = model(img.permute(2, 0, 1)[None].contiguous(), None, mode='predict')[0]
    want = ref.seg_logits.data.cpu().softmax(0)
    err = (out[0].seg_logits.data.cpu() - want).abs().max().item()
    print(f'single view [{be.dev.type}]: max |prob - softmax(predict)| = {err:.3e}')
    assert err <= PROB_TOL
    _check_mask(out[0].pred_sem_seg.data.cpu()[0], want, 'single view')


def test_seg_tta_model_is_registered_and_refuses_binary_heads(be):
    import led_net_amd as L
    assert L.MODELS.get('SegTTAModel') is L.SegTTAModel
    cfg = L.load_config(CFG)['model']
    m = L.MODELS.build(dict(type='SegTTAModel', module=cfg))
    assert isinstance(m.module, L.EncoderDecoder)
    m.module.out_channels = 1
    with pytest.raises(NotImplementedError):
        L.SegTTAModel(module=m.module)


# ---- 8. invalid arguments are refused before any launch ---------------------------------------------------------------------
def test_invalid_arguments_raise(be):
    import ctypes as C
    from led_net_amd import _lib, ops
    z = lambda *s, **k: torch.zeros(s, device=be.dev, **k)
    with pytest.raises(ops.LednError):
        ops.tta_accumulate(z(8, 8, 7), z(7, 8, 8), first=True, last=True, K=1)                  # unsupported C
    with pytest.raises(ops.LednError):
        ops.tta_accumulate(z(8, 8, 19), z(2, 8, 8), first=True, last=True, K=1)                 # class mismatch
    with pytest.raises(ops.LednError):
        ops.tta_accumulate(z(8, 8, 19), z(19, 8, 8), first=True, last=True, K=1, valid=(9, 8))  # valid outside src
    with pytest.raises(ops.LednError):
        ops.tta_accumulate(z(8, 8, 19), z(19, 8, 8), first=True, last=True, K=1, mask=z(8, 9, dtype=torch.uint8))
    with pytest.raises(ops.LednError):
        ops.slide_accumulate(z(1, 19, 16, 16), z(1, 8, 8, 19), 9, 0)                            # window outside
    with pytest.raises(ops.LednError):
        ops.slide_accumulate(z(1, 19, 16, 16), z(2, 8, 8, 19), 0, 0)                            # batch mismatch
    with pytest.raises(ops.LednError):
        ops.slide_accumulate(z(1, 7, 16, 16), z(1, 8, 8, 7), 0, 0)
    ones = torch.ones(16, dtype=torch.int32)
    with pytest.raises(ops.LednError, match='count 0'):
        ops.slide_finish(z(1, 19, 16, 16), torch.cat([ones[:15], ones[:1] * 0]), ones)
    with pytest.raises(ops.LednError):
        ops.slide_finish(z(1, 19, 16, 16), ones[:15], ones)
    # the C ABI itself: LEDN_EINVAL, nothing launched
    lib = _lib.get_lib()
    a, s = z(7, 8, 8), z(8, 8, 7)
    d = _lib.TtaDesc()
    d.src, d.acc, d.Hs, d.Ws, d.hv, d.wv, d.C, d.Ho, d.Wo, d.first, d.last, d.K = s.data_ptr(), a.data_ptr(), 8, 8, 8, 8, 7, 8, 8, 1, 1, 1
    assert lib.cdll.ledn_tta_accumulate(C.byref(d), None) == _lib.EINVAL
    d.C, d.hv = 19, 9
    assert lib.cdll.ledn_tta_accumulate(C.byref(d), None) == _lib.EINVAL
    assert lib.cdll.ledn_slide_accumulate(a.data_ptr(), s.data_ptr(), 1, 19, 8, 8, 4, 0, 8, 8, 0, None) == _lib.EINVAL
    assert lib.cdll.ledn_slide_finish(a.data_ptr(), None, None, None, 1, 19, 8, 8, None) == _lib.EINVAL


# ---- 9. tools/test.py --tta ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_test_cli_with_and_without_tta(tmp_path):
    import led_net_amd as L
    torch.manual_seed(11)
    model = L.MODELS.build(L.load_config(CFG)['model'])
    ck = str(tmp_path / 'w.pth')
    torch.save(dict(state_dict=model.state_dict(), meta=dict(iter=0)), ck)
    # (the issue's 128 x 256 is below what the network's GETB stage accepts, on the parent commit too: the 0.5 x view
    # of 576 x 640 is the smallest size class that runs)
    args = ['tools/test.py', CFG, ck, '--num-images', '2', '--height', '576', '--width', '640']
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(extra):
        r = subprocess.run([sys.executable] + args + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f'{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
        return r.stdout
    out = run(['--tta'])
    assert 'per class results' in out and re.search(r'aAcc: ([0-9.]+)\s+mIoU: ([0-9.]+)\s+mAcc: ([0-9.]+)', out), out[-600:]
    # without the flag: exactly the lines of the loop the script has always run (predict -> IoUMetric), recomputed here
    plain = run([])
    dev = torch.device('cuda:0')
    m = L.init_model(CFG, ck, device=dev)
    m.set_act_dtype(torch.bfloat16)
    metric = L.IoUMetric(2, 255, ['mIoU'])
    g = torch.Generator().manual_seed(304)
    img = torch.randint(0, 256, (2, 3, 576, 640), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 2, (2, 576, 640), dtype=torch.int64, generator=g).to(dev)
    with torch.no_grad():
        res = m(img, None, mode='predict')
    metric.process([o.pred_sem_seg.data for o in res], [lab[j] for j in range(2)])
    summary, per_class = metric.compute_metrics()
    classes = getattr(m, 'dataset_meta', {}).get('classes') or ['0', '1']
    want = ['per class results:'] + [f'  {classes[c]:>12s}  IoU {per_class["IoU"][c] * 100:6.2f}  Acc {per_class["Acc"][c] * 100:6.2f}'
                                     for c in range(2)] + ['  '.join(f'{k}: {v:.2f}' for k, v in summary.items())]
    assert plain.splitlines() == want
