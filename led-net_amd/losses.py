"""OhemCrossEntropy (registered under the reference's name) and accuracy.

Mirrors mmseg/models/losses/ohem_cross_entropy_loss.py:11-94 (constructor
arguments, ``loss_name`` property, selection semantics) and
losses/accuracy.py:6-60 (top-1, ignore_index).  The arithmetic runs in the
fused HIP kernels of csrc/attn_loss_opt.hip (ohem_*: softmax prob + CE, exact k-th
smallest by radix select, masked mean, backward).  ``class_weight`` (ohem_cross_entropy_loss.py:42,63-73: the
``weight`` of F.cross_entropy) scales the per-pixel losses and gradients inside those kernels; it does not take part
in the selection, and the mean still divides by the number of selected pixels.
"""
import math

import torch
import torch.nn as nn

from .registry import MODELS


@MODELS.register_module()
class OhemCrossEntropy(nn.Module):
    def __init__(self, ignore_label=255, thres=0.7, min_kept=100000, loss_weight=1.0,
                 class_weight=None, loss_name='loss_ohem'):
        super().__init__()
        if class_weight is not None:
            if isinstance(class_weight, str) or not isinstance(class_weight, (list, tuple)):
                raise TypeError('class_weight must be a list or tuple of floats (one per class) or None')
            if not class_weight or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in class_weight):
                raise ValueError('class_weight must hold one finite number per class')
        self.class_weight = class_weight            # as the reference keeps it (the list from the config)
        # its device copy: not persistent, so state_dict() keeps the reference's key set; model.to(dev) moves it
        self.register_buffer('_class_weight', None if class_weight is None else
                             torch.tensor([float(v) for v in class_weight], dtype=torch.float32), persistent=False)
        self.thresh = thres
        self.min_kept = max(1, min_kept)
        self.ignore_label = ignore_label
        self.loss_weight = loss_weight
        self.loss_name_ = loss_name

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

    def forward(self, score, target):
        """score: N x C x H x W (any float layout), target: N x H x W int64."""
        from .train import ohem_loss
        return ohem_loss(self, score, target)

    @property
    def loss_name(self):
        return self.loss_name_


def build_loss(cfg):
    return MODELS.build(cfg)
