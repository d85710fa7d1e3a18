"""OhemCrossEntropy, CrossEntropyLoss and DiceLoss (registered under the reference's names) and accuracy.

Mirrors mmseg/models/losses/ohem_cross_entropy_loss.py:11-94 (constructor
arguments, ``loss_name`` property, selection semantics) and
losses/accuracy.py:6-60 (top-1, ignore_index).  The arithmetic runs in the
fused HIP kernels of csrc/attn_loss_opt.hip (ohem_*: softmax prob + CE, exact k-th
smallest by radix select, masked mean, backward).  ``class_weight`` (ohem_cross_entropy_loss.py:42,63-73: the
``weight`` of F.cross_entropy) scales the per-pixel losses and gradients inside those kernels; it does not take part
in the selection, and the mean still divides by the number of selected pixels.

CrossEntropyLoss (softmax form) and DiceLoss mirror losses/cross_entropy_loss.py:211-311 and losses/dice_loss.py:94-202:
constructor signatures, ``loss_name``, an empty state_dict.  Their arithmetic runs in csrc/seg_loss.hip (one streaming
pass + a fixed-order finish, the divisor formed on the device, nothing per-pixel stored); see DESIGN.md
"CrossEntropyLoss and DiceLoss in the head" for the layouts and the two deviations from the reference.
"""
import math

import torch
import torch.nn as nn

from .registry import MODELS


def _checked_class_weight(class_weight):
    if class_weight is not None:
        if isinstance(class_weight, str) or not isinstance(class_weight, (list, tuple)):
            raise TypeError('class_weight must be a list or tuple of floats (one per class) or None')
        if not class_weight or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in class_weight):
            raise ValueError('class_weight must hold one finite number per class')
    return class_weight


class _ClassWeighted(nn.Module):
    """a loss with the reference's ``class_weight`` list and its device copy for the kernels"""

    def _set_class_weight(self, class_weight):
        self.class_weight = _checked_class_weight(class_weight)      # as the reference keeps it (the list from the config)
        # its device copy: not persistent, so state_dict() keeps the reference's key set; model.to(dev) moves it
        self.register_buffer('_class_weight', None if class_weight is None else
                             torch.tensor([float(v) for v in class_weight], dtype=torch.float32), persistent=False)

    def class_weight_on(self, logits):
        """the class weights as the kernels take them (None, or the [C] f32 buffer on the logits' device), checked
        against the class count of channels-last `logits`"""
        w = self._class_weight
        if w is None:
            return None
        if w.numel() != logits.shape[-1]:
            raise ValueError(f'{self.loss_name}: class_weight has {w.numel()} entries but the logits have '
                             f'{logits.shape[-1]} classes')
        if w.device != logits.device:
            raise RuntimeError(f'{self.loss_name}: class_weight is on {w.device}, the logits on {logits.device} '
                               f'(move the module with .to(device))')
        return w


@MODELS.register_module()
class OhemCrossEntropy(_ClassWeighted):
    def __init__(self, ignore_label=255, thres=0.7, min_kept=100000, loss_weight=1.0,
                 class_weight=None, loss_name='loss_ohem'):
        super().__init__()
        self._set_class_weight(class_weight)
        self.thresh = thres
        self.min_kept = max(1, min_kept)
        self.ignore_label = ignore_label
        self.loss_weight = loss_weight
        self.loss_name_ = loss_name

    def forward(self, score, target):
        """score: N x C x H x W (any float layout), target: N x H x W int64."""
        from .train import ohem_loss
        return ohem_loss(self, score, target)

    @property
    def loss_name(self):
        return self.loss_name_


def _checked_reduction(who, reduction):
    if reduction not in ('mean', 'sum'):
        raise NotImplementedError(f"{who}: reduction={reduction!r} is not supported ('mean' or 'sum': the loss kernels "
                                  f'reduce on the device and keep nothing per pixel)')
    return reduction


@MODELS.register_module()
class CrossEntropyLoss(_ClassWeighted):
    """losses/cross_entropy_loss.py:211-311, the softmax form (``cross_entropy``, :12-78)."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction='mean', class_weight=None, loss_weight=1.0,
                 loss_name='loss_ce', avg_non_ignore=False):
        super().__init__()
        if use_sigmoid:
            raise NotImplementedError('CrossEntropyLoss: use_sigmoid=True (binary cross-entropy) is not supported')
        if use_mask:
            raise NotImplementedError('CrossEntropyLoss: use_mask=True (mask cross-entropy) is not supported')
        if isinstance(class_weight, str):
            raise TypeError(f'CrossEntropyLoss: class_weight={class_weight!r}: a file path is not supported, give the '
                            f'list of weights')
        self.use_sigmoid, self.use_mask = False, False
        self.reduction = _checked_reduction('CrossEntropyLoss', reduction)
        self.loss_weight = loss_weight
        self._set_class_weight(class_weight)
        self.avg_non_ignore = avg_non_ignore
        self._loss_name = loss_name

    def extra_repr(self):
        return f'avg_non_ignore={self.avg_non_ignore}'

    def kernel_args(self, logits, ignore_index):
        """(family, keyword arguments of ops_train.ce_loss*_fwd, of *_bwd) for channels-last `logits`"""
        bwd = dict(loss_weight=self.loss_weight, ignore_index=ignore_index, class_weight=self.class_weight_on(logits))
        return 'ce', dict(bwd, reduction=self.reduction, avg_non_ignore=self.avg_non_ignore), bwd

    def forward(self, cls_score, label, ignore_index=-100):
        """cls_score: N x C x H x W (any float layout), label: N x H x W int64."""
        from .train import seg_loss
        return seg_loss(self, cls_score, label, ignore_index)

    @property
    def loss_name(self):
        return self._loss_name


@MODELS.register_module()
class DiceLoss(nn.Module):
    """losses/dice_loss.py:94-202.  ``ignore_index`` is the reference's class-CHANNEL drop (dice_loss.py:69-72): a
    value in [0, C) removes that class from the sums, the default 255 removes nothing, and a pixel LABELLED 255 keeps
    its predictions in the denominator (its one-hot row is all zeros)."""

    def __init__(self, use_sigmoid=True, activate=True, reduction='mean', naive_dice=False, loss_weight=1.0,
                 ignore_index=255, eps=1e-3, loss_name='loss_dice'):
        super().__init__()
        if not activate:
            raise NotImplementedError('DiceLoss: activate=False (predictions that are already probabilities) is not '
                                      'supported')
        self.use_sigmoid = use_sigmoid
        self.reduction = _checked_reduction('DiceLoss', reduction)
        self.naive_dice = naive_dice
        self.loss_weight = loss_weight
        self.eps = eps
        self.activate = activate
        self.ignore_index = ignore_index
        self._loss_name = loss_name

    def kernel_args(self, logits, ignore_index):
        """(family, keyword arguments of ops_train.dice_loss*_fwd, of *_bwd); `ignore_index`: the label the accuracy
        leaves out (the loss itself does not see it)"""
        bwd = dict(loss_weight=self.loss_weight, use_sigmoid=self.use_sigmoid, naive_dice=self.naive_dice,
                   ignore_class=self.ignore_index, eps=self.eps, reduction=self.reduction)
        return 'dice', dict(bwd, acc_ignore_index=ignore_index), bwd

    def forward(self, pred, target, ignore_index=255):
        """pred: N x C x H x W (any float layout), target: N x H x W int64."""
        from .train import seg_loss
        return seg_loss(self, pred, target, ignore_index)

    @property
    def loss_name(self):
        return self._loss_name


def build_loss(cfg):
    return MODELS.build(cfg)
