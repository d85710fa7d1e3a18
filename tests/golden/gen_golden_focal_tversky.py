#!/usr/bin/env python3
"""Golden vectors for FocalLoss and TverskyLoss, from the reference checkout (gen_golden_class_weight.REF), IMPORTED
and run on seeded logits and labels.  Only data is written (tests/golden/g23_*.npz: in/score, in/target, out/loss,
out/acc, gin/score (d score by autograd), meta with the class name, the constructor kwargs and the call's
ignore_index); re-run: python tests/golden/gen_golden_focal_tversky.py

TverskyLoss: the reference's own class (mmseg/models/losses/tversky_loss.py:60-137), called as the head calls it.

FocalLoss: NOT the class's forward.  Off the GPU FocalLoss.forward (focal_loss.py:286-297) indexes
target[:, num_classes] and fails; its GPU branch (:272-285) needs mmcv's compiled op.  The fixtures therefore call the
reference's own py_sigmoid_focal_loss (:13-68: the same arithmetic as the op, by the file's own account) on exactly what
forward's GPU branch builds: the [B,C,H,W] -> [N,C] flattening (:241-248), valid_mask = (target != ignore_index) and
ignored labels set to 0 (:262-266), one_hot(target, C + 1)[:, :C] (:274-280), then loss_weight * (...) (:299).  Those
statements are restated in focal_forward below, around the imported function.

Import plumbing (as gen_golden_seg_losses.py): parent packages are empty modules whose __path__ points at the
reference directories; NAME-ONLY stand-ins for mmseg.registry.MODELS / mmseg.models.builder.LOSSES (register_module),
mmengine.fileio.load and mmcv.ops.sigmoid_focal_loss (never called).
"""
import os
import sys
import warnings

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_class_weight import REF, _pkg, sibling_class_weight  # noqa: E402
from gen_golden_seg_losses import install_all, save  # noqa: E402


def install_more():
    install_all()

    def sigmoid_focal_loss(*a, **k):
        raise RuntimeError('mmcv.ops.sigmoid_focal_loss: stand-in, not callable')
    _pkg('mmcv')
    _pkg('mmcv.ops', sigmoid_focal_loss=sigmoid_focal_loss)
    _pkg('mmseg.models.builder', LOSSES=sys.modules['mmseg.registry'].MODELS)


def focal_forward(py_sigmoid_focal_loss, pred, target, ignore_index, gamma=2.0, alpha=0.5, reduction='mean',
                  class_weight=None, loss_weight=1.0):
    """FocalLoss.forward's GPU branch (focal_loss.py:241-284,299-309) around the reference's py_sigmoid_focal_loss"""
    pred = pred.transpose(0, 1)
    pred = pred.reshape(pred.size(0), -1)
    pred = pred.transpose(0, 1).contiguous()
    target = target.view(-1).contiguous()
    valid_mask = (target != ignore_index).view(-1, 1)
    target = torch.where(target == ignore_index, target.new_tensor(0), target)
    num_classes = pred.size(1)
    one_hot_target = F.one_hot(target, num_classes=num_classes + 1)[:, :num_classes]
    return loss_weight * py_sigmoid_focal_loss(pred, one_hot_target, None, None, gamma=gamma, alpha=alpha,
                                               class_weight=class_weight, valid_mask=valid_mask, reduction=reduction,
                                               avg_factor=None)


def main():
    install_more()
    assert os.path.isdir(REF)
    from mmseg.models.losses.focal_loss import FocalLoss, py_sigmoid_focal_loss
    from mmseg.models.losses.tversky_loss import TverskyLoss
    from mmseg.models.losses.accuracy import accuracy
    w19 = sibling_class_weight()
    # name, class, kwargs, ignore_index of the call, (N, C, H, W), share of labels 255, logit scale
    cases = [
        ('g23_focal_default', 'FocalLoss', dict(), 255, (2, 2, 64, 64), 0.12, 3.0),
        ('g23_focal_gamma0', 'FocalLoss', dict(gamma=0.0), 255, (2, 2, 64, 64), 0.15, 3.0),
        ('g23_focal_g15_a25', 'FocalLoss', dict(gamma=1.5, alpha=0.25), 255, (2, 2, 64, 64), 0.12, 3.0),
        ('g23_focal_alpha_list', 'FocalLoss', dict(alpha=[0.25, 0.6]), 255, (2, 2, 64, 64), 0.18, 3.0),
        ('g23_focal_cw', 'FocalLoss', dict(class_weight=[0.7, 1.6]), 255, (2, 2, 64, 64), 0.12, 3.0),
        ('g23_focal_sum_w04', 'FocalLoss', dict(reduction='sum', loss_weight=0.4), 255, (2, 5, 32, 32), 0.12, 2.0),
        ('g23_focal_c19', 'FocalLoss', dict(class_weight=w19, alpha=0.25), 255, (1, 19, 40, 40), 0.12, 2.0),
        ('g23_focal_all_ignored', 'FocalLoss', dict(), 255, (1, 2, 16, 16), 1.0, 1.0),
        ('g23_tversky_default', 'TverskyLoss', dict(), 255, (2, 2, 64, 64), 0.12, 3.0),
        ('g23_tversky_half_cw', 'TverskyLoss', dict(alpha=0.5, beta=0.5, smooth=0.1, class_weight=[0.7, 1.6]), 255,
         (2, 2, 64, 64), 0.15, 3.0),
        ('g23_tversky_skip_class0', 'TverskyLoss', dict(ignore_index=0), 255, (2, 2, 64, 64), 0.12, 3.0),
        ('g23_tversky_c5', 'TverskyLoss', dict(loss_weight=0.4), 255, (2, 5, 32, 32), 0.18, 2.0),
        ('g23_tversky_c19', 'TverskyLoss', dict(class_weight=w19), 255, (1, 19, 40, 40), 0.12, 2.0),
        ('g23_tversky_all_ignored', 'TverskyLoss', dict(), 255, (1, 2, 16, 16), 1.0, 1.0),
    ]
    g = torch.Generator().manual_seed(2300)
    for name, kind, kw, ign_idx, shp, p_ign, scale in cases:
        n, c, h, w = shp
        score = (scale * torch.randn(shp, generator=g)).requires_grad_(True)
        tgt = torch.randint(0, c, (n, h, w), generator=g)
        ign = torch.rand((n, h, w), generator=g) < p_ign
        tgt[ign] = 255
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if kind == 'FocalLoss':
                crit = FocalLoss(**kw)          # (the constructor's checks; its forward is not callable here)
                loss = focal_forward(py_sigmoid_focal_loss, score, tgt, ign_idx, gamma=crit.gamma, alpha=crit.alpha,
                                     reduction=crit.reduction, class_weight=crit.class_weight,
                                     loss_weight=crit.loss_weight)
            else:
                loss = TverskyLoss(**kw)(score, tgt, ignore_index=ign_idx)
        loss.backward()
        acc = accuracy(score.detach(), tgt, ignore_index=255)
        save(name, {'score': score.detach(), 'target': tgt}, {'loss': loss.detach(), 'acc': acc}, {'score': score.grad},
             dict(kind=kind, kwargs=kw, ignore_index=ign_idx))


if __name__ == '__main__':
    main()
