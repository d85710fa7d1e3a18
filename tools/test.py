#!/usr/bin/env python3
"""Evaluation entry point with the reference's command line (tools/test.py: CONFIG CHECKPOINT [--work-dir])
on the built-in loop: `mode='predict'` -> uint8 argmax masks (fused into the last resize) -> IoUMetric
histograms on the device (ledn_iou_hist) -> the aAcc / mIoU / mAcc summary of the reference's IoUMetric.
Datasets are out of scope: images and labels are synthetic.

    python tools/test.py CONFIG CHECKPOINT [--num-images 32] [--height 1024 --width 1024] [--tta]

--tta: the reference's `tools/test.py --tta` -- every image goes through the cityscapes `tta_pipeline` (six scales x
{no flip, horizontal flip} = 12 views, configs/_base_/datasets/cityscapes.py:26-41) and `SegTTAModel` merges the views'
softmax at the original size; same metric output.
"""
import argparse
import os.path as osp
import sys

import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
import led_net_amd as L  # noqa: E402


def main():
    p = argparse.ArgumentParser(description='Test (and eval) LED-Net (HIP)')
    p.add_argument('config')
    p.add_argument('checkpoint')
    p.add_argument('--work-dir')
    p.add_argument('--num-images', type=int, default=32)
    p.add_argument('--batch-size', type=int, default=8)
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=1024)
    p.add_argument('--tta', action='store_true', help='Test time augmentation')
    args = p.parse_args()
    dev = torch.device('cuda:0')
    model = L.init_model(args.config, args.checkpoint if osp.exists(args.checkpoint) else None, device=dev)
    model.set_act_dtype(torch.bfloat16)
    ncls = model.decode_head.num_classes
    metric = L.IoUMetric(ncls, 255, ['mIoU'])
    if args.tta:
        img_ratios = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]
        tta = L.transforms.TestTimeAug(transforms=[
            [dict(type='Resize', scale_factor=r, keep_ratio=True) for r in img_ratios],
            [dict(type='RandomFlip', prob=0., direction='horizontal'), dict(type='RandomFlip', prob=1., direction='horizontal')],
            [dict(type='LoadAnnotations')], [dict(type='PackSegInputs')]])
        tta_model = L.MODELS.build(dict(type='SegTTAModel', module=model))
    g = torch.Generator().manual_seed(304)
    for i in range(0, args.num_images, args.batch_size):
        n = min(args.batch_size, args.num_images - i)
        img = torch.randint(0, 256, (n, 3, args.height, args.width), dtype=torch.uint8, generator=g).to(dev)
        lab = torch.randint(0, ncls, (n, args.height, args.width), dtype=torch.int64, generator=g).to(dev)
        if args.tta:
            packed = [tta.transform(dict(img=img[j].permute(1, 2, 0).contiguous(), ori_shape=(args.height, args.width)))
                      for j in range(n)]
            out = tta_model.test_step(L.transforms.collate_views(packed))
        else:
            with torch.no_grad():
                out = model(img, None, mode='predict')
        metric.process([o.pred_sem_seg.data for o in out], [lab[j] for j in range(n)])
    summary, per_class = metric.compute_metrics()
    classes = getattr(model, 'dataset_meta', {}).get('classes') or [str(c) for c in range(ncls)]
    print('per class results:')
    for c in range(ncls):
        print(f'  {classes[c]:>12s}  IoU {per_class["IoU"][c] * 100:6.2f}  Acc {per_class["Acc"][c] * 100:6.2f}')
    print('  '.join(f'{k}: {v:.2f}' for k, v in summary.items()))


if __name__ == '__main__':
    main()
