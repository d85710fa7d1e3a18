"""OhemCrossEntropy, CrossEntropyLoss, DiceLoss, FocalLoss, TverskyLoss, LovaszLoss and HuasdorffDisstanceLoss (registered
under the reference's names)
and accuracy.

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

FocalLoss (sigmoid form) and TverskyLoss mirror losses/focal_loss.py:136-337 and losses/tversky_loss.py:60-137 in the
same way, on further kernels of csrc/seg_loss.hip; DESIGN.md "FocalLoss and TverskyLoss in the head".

LovaszLoss (the multi-class Lovasz-Softmax form) mirrors losses/lovasz_loss.py:225-323; its arithmetic is the on-device
radix sort and closed-form Lovasz gradient of csrc/lovasz.hip; DESIGN.md "LovaszLoss in the head".

HuasdorffDisstanceLoss mirrors losses/huasdorff_distance_loss.py:77-160 on the exact on-device distance transform of
csrc/hausdorff.hip; DESIGN.md "HuasdorffDisstanceLoss in the head".
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


@MODELS.register_module()
class FocalLoss(_ClassWeighted):
    """losses/focal_loss.py:136-337, the sigmoid form as FocalLoss.forward's GPU branch computes it (:241-284 + the
    arithmetic of py_sigmoid_focal_loss, :45-67).  'mean' divides by N*H*W*C: ignored pixels stay in the divisor.  A
    label outside [0, C) that is not ``ignore_index`` has an all-zero target row (the reference gets that far only for
    label == C)."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.5, reduction='mean', class_weight=None, loss_weight=1.0,
                 loss_name='loss_focal'):
        super().__init__()
        if use_sigmoid is not True:
            raise NotImplementedError('FocalLoss: use_sigmoid=False is not supported (only the sigmoid form exists)')
        if isinstance(class_weight, str):
            raise TypeError(f'FocalLoss: class_weight={class_weight!r}: a file path is not supported, give the list '
                            f'of weights')
        if isinstance(alpha, (list, tuple)):
            if not alpha or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in alpha):
                raise ValueError('FocalLoss: alpha must be a float or a list of one finite number per class')
        elif not isinstance(alpha, (int, float)) or isinstance(alpha, bool) or not math.isfinite(alpha):
            raise TypeError(f'FocalLoss: alpha={alpha!r} must be a float or a list of floats')
        if not isinstance(gamma, (int, float)) or isinstance(gamma, bool) or not gamma >= 0:
            raise ValueError(f'FocalLoss: gamma={gamma!r} must be a number >= 0')
        self.use_sigmoid = True
        self.gamma = gamma
        self.alpha = alpha
        self.reduction = _checked_reduction('FocalLoss', reduction)
        self.loss_weight = loss_weight
        self._set_class_weight(class_weight)
        # (a list's device copy, like class_weight's: not persistent, the state_dict stays empty)
        self.register_buffer('_alpha', torch.tensor([float(v) for v in alpha], dtype=torch.float32)
                             if isinstance(alpha, (list, tuple)) else None, persistent=False)
        self._loss_name = loss_name

    def alpha_on(self, logits):
        """alpha as the kernels take it: the float, or the [C] f32 buffer, checked against channels-last `logits`"""
        a = self._alpha
        if a is None:
            return float(self.alpha)
        if a.numel() != logits.shape[-1]:
            raise ValueError(f'{self.loss_name}: alpha has {a.numel()} entries but the logits have '
                             f'{logits.shape[-1]} classes')
        if a.device != logits.device:
            raise RuntimeError(f'{self.loss_name}: alpha is on {a.device}, the logits on {logits.device} (move the '
                               f'module with .to(device))')
        return a

    def kernel_args(self, logits, ignore_index):
        """(family, keyword arguments of ops_train.focal_loss*_fwd, of *_bwd) for channels-last `logits`"""
        kw = dict(loss_weight=self.loss_weight, gamma=self.gamma, alpha=self.alpha_on(logits), ignore_index=ignore_index,
                  class_weight=self.class_weight_on(logits), reduction=self.reduction)
        return 'focal', kw, kw

    def forward(self, pred, target, ignore_index=255):
        """pred: N x C x H x W (any float layout), target: N x H x W int64."""
        from .train import seg_loss
        return seg_loss(self, pred, target, ignore_index)

    @property
    def loss_name(self):
        return self._loss_name


@MODELS.register_module()
class TverskyLoss(_ClassWeighted):
    """losses/tversky_loss.py:60-137.  ``ignore_index`` is the loss's own: pixels LABELLED so are masked out of the
    sums and the class of that index is left out of the loss (which is still divided by C); the ``ignore_index`` of the
    call only selects the pixels of the reported accuracy, as the reference's forward ignores it.  2 to 32 classes.
    ``smooth=0`` is accepted as the reference accepts it: an image without a valid pixel then gives 0 / 0 = NaN."""

    def __init__(self, smooth=1, class_weight=None, loss_weight=1.0, ignore_index=255, alpha=0.3, beta=0.7,
                 loss_name='loss_tversky'):
        super().__init__()
        if isinstance(class_weight, str):
            raise TypeError(f'TverskyLoss: class_weight={class_weight!r}: a file path is not supported, give the list '
                            f'of weights')
        if not alpha + beta == 1.0:
            raise ValueError(f'TverskyLoss: alpha + beta must be 1.0 (alpha={alpha!r}, beta={beta!r})')
        if not smooth >= 0:
            raise ValueError(f'TverskyLoss: smooth={smooth!r} must be >= 0')
        self.smooth = smooth
        self._set_class_weight(class_weight)
        self.loss_weight = loss_weight
        self.ignore_index = ignore_index
        self.alpha = alpha
        self.beta = beta
        self._loss_name = loss_name

    def kernel_args(self, logits, ignore_index):
        """(family, keyword arguments of ops_train.tversky_loss*_fwd, of *_bwd); `ignore_index`: the label the accuracy
        leaves out"""
        from .ops_train import TVERSKY_MAX_CLASSES
        if logits.shape[-1] > TVERSKY_MAX_CLASSES:
            raise ValueError(f'{self.loss_name}: {logits.shape[-1]} classes; TverskyLoss takes at most '
                             f'{TVERSKY_MAX_CLASSES}')
        fwd = dict(loss_weight=self.loss_weight, alpha=self.alpha, beta=self.beta, smooth=self.smooth,
                   ignore_index=self.ignore_index, class_weight=self.class_weight_on(logits),
                   acc_ignore_index=ignore_index)
        return 'tversky', fwd, dict(ignore_index=self.ignore_index)

    def forward(self, pred, target, ignore_index=255, **kwargs):
        """pred: N x C x H x W (any float layout), target: N x H x W int64."""
        from .train import seg_loss
        return seg_loss(self, pred, target, ignore_index)

    @property
    def loss_name(self):
        return self._loss_name


@MODELS.register_module()
class LovaszLoss(_ClassWeighted):
    """losses/lovasz_loss.py:225-323, ``loss_type='multi_class'`` (lovasz_softmax, :129-222).  As in the reference,
    ``per_image=False`` requires ``reduction='none'`` (:269-271; the result is a scalar anyway) and ranks the valid
    pixels of the whole batch; ``per_image=True`` ranks each image on its own and takes the 'mean' or 'sum' of the N
    losses.  Without a valid pixel (in the batch, or in one image) that loss is 0, where the reference returns an empty
    tensor or fails."""

    def __init__(self, loss_type='multi_class', classes='present', per_image=False, reduction='mean', class_weight=None,
                 loss_weight=1.0, loss_name='loss_lovasz'):
        super().__init__()
        if loss_type == 'binary':
            raise NotImplementedError("LovaszLoss: loss_type='binary' (the hinge form on a one-channel head) is not "
                                      "supported; use loss_type='multi_class'")
        if loss_type != 'multi_class':
            raise ValueError(f"LovaszLoss: loss_type={loss_type!r} should be 'binary' or 'multi_class'")
        if isinstance(classes, str):
            if classes not in ('all', 'present'):
                raise ValueError(f"LovaszLoss: classes={classes!r} must be 'all', 'present' or a list of class indices")
        elif (not isinstance(classes, (list, tuple)) or not classes
              or not all(isinstance(c, int) and not isinstance(c, bool) and c >= 0 for c in classes)
              or len(set(classes)) != len(classes)):
            raise ValueError(f"LovaszLoss: classes={classes!r} must be 'all', 'present' or a non-empty list of distinct "
                             f'class indices')
        if per_image:
            if reduction == 'none':
                raise NotImplementedError("LovaszLoss: reduction='none' with per_image=True (one loss per image) is not "
                                          "supported; use 'mean' or 'sum'")
            if reduction not in ('mean', 'sum'):
                raise ValueError(f"LovaszLoss: reduction={reduction!r} must be 'mean' or 'sum' with per_image=True")
        elif reduction != 'none':
            raise ValueError(f"LovaszLoss: reduction={reduction!r}: mmseg requires reduction='none' when per_image is "
                             f'False (the loss is a scalar either way)')
        if isinstance(class_weight, str):
            raise TypeError(f'LovaszLoss: class_weight={class_weight!r}: a file path is not supported, give the list '
                            f'of weights')
        self.loss_type = loss_type
        self.classes = list(classes) if isinstance(classes, tuple) else classes
        self.per_image = bool(per_image)
        self.reduction = reduction
        self.loss_weight = loss_weight
        self._set_class_weight(class_weight)
        self._loss_name = loss_name

    def extra_repr(self):
        return f'classes={self.classes!r}, per_image={self.per_image}, reduction={self.reduction!r}'

    def kernel_args(self, logits, ignore_index):
        """(family, keyword arguments of ops_train.lovasz_loss_fwd, of lovasz_loss_bwd) for channels-last `logits`"""
        Cc = logits.shape[-1]
        if not isinstance(self.classes, str) and not all(c < Cc for c in self.classes):
            raise ValueError(f'{self.loss_name}: classes={self.classes!r} but the logits have {Cc} classes')
        fwd = dict(loss_weight=self.loss_weight, classes=self.classes, per_image=self.per_image,
                   reduction='mean' if self.reduction == 'none' else self.reduction, ignore_index=ignore_index,
                   class_weight=self.class_weight_on(logits))
        return 'lovasz', fwd, {}

    def forward(self, cls_score, label, ignore_index=255, **kwargs):
        """cls_score: N x C x H x W (any float layout), label: N x H x W int64."""
        from .train import seg_loss
        return seg_loss(self, cls_score, label, ignore_index)

    @property
    def loss_name(self):
        return self._loss_name


@MODELS.register_module()
class HuasdorffDisstanceLoss(nn.Module):
    """losses/huasdorff_distance_loss.py:77-160 (the reference's spelling, so that its configs load).  The loss's own
    ``ignore_index`` is the constructor's: the reference swallows a call-time ``ignore_index`` in ``**kwargs``; those
    pixels become background with target 0 and stay in the mean.  'mean', 'sum' and 'none' give the same scalar (the
    reference reduces a scalar).  ``class_weight`` is rejected: the reference's own check of it
    (``class_weight.ndim == num_class``) fails for every weight vector."""

    def __init__(self, reduction='mean', class_weight=None, loss_weight=1.0, ignore_index=255,
                 loss_name='loss_huasdorff_disstance', **kwargs):
        super().__init__()
        if isinstance(class_weight, str):
            raise TypeError(f'HuasdorffDisstanceLoss: class_weight={class_weight!r}: a file path is not supported')
        if class_weight is not None:
            raise NotImplementedError('HuasdorffDisstanceLoss: class_weight is not supported (the reference asserts '
                                      'class_weight.ndim == num_class, which no weight vector passes)')
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError(f"HuasdorffDisstanceLoss: reduction={reduction!r} must be 'none', 'mean' or 'sum'")
        self.reduction = reduction
        self.class_weight = None
        self.loss_weight = loss_weight
        self.ignore_index = 255 if ignore_index is None else int(ignore_index)
        self._loss_name = loss_name

    def extra_repr(self):
        return f'reduction={self.reduction!r}, ignore_index={self.ignore_index}, loss_weight={self.loss_weight}'

    def kernel_args(self, logits, ignore_index):
        """(family, keyword arguments of ops_train.hausdorff_loss_fwd, of hausdorff_loss_bwd) for channels-last
        `logits`; ignore_index: the head's, which the accuracy uses -- the loss uses the constructor's"""
        Cc = logits.shape[-1]
        if 1 <= self.ignore_index < Cc:
            raise ValueError(f'{self.loss_name}: ignore_index={self.ignore_index} is one of the {Cc} classes of the loss '
                             f'(the reference then repeats the previous class\'s term by accident)')
        return 'hausdorff', dict(loss_weight=self.loss_weight, ignore_index=self.ignore_index,
                                 acc_ignore_index=ignore_index), {}

    def forward(self, pred, target, ignore_index=255, **kwargs):
        """pred: N x C x H x W (any float layout), target: N x H x W int64.  ``ignore_index`` here is what the accuracy
        leaves out (the loss keeps the constructor's); ``avg_factor`` is not supported."""
        if kwargs.get('avg_factor') is not None:
            raise NotImplementedError(f'{self.loss_name}: avg_factor is not supported')
        if kwargs.get('reduction_override') not in (None, 'none', 'mean', 'sum'):
            raise ValueError(f"{self.loss_name}: reduction_override={kwargs['reduction_override']!r}")
        from .train import seg_loss
        return seg_loss(self, pred, target, ignore_index)

    @property
    def loss_name(self):
        return self._loss_name


def build_loss(cfg):
    return MODELS.build(cfg)
