"""led-net_amd: MI355X-native LED-Net forward/backward hot path.

Public surface = the reference's plugin names:
``MODELS.build(dict(type='LEDNet'|'LEDHead'|'OhemCrossEntropy'|'CrossEntropyLoss'|'DiceLoss'|'FocalLoss'|
'TverskyLoss'|'LovaszLoss'|'HuasdorffDisstanceLoss'|'EncoderDecoder'|'SegTTAModel', ...))``.
Compute is in csrc/libledn_hip.so (C ABI: include/ledn.h); there is no CPU path.
"""
from . import _lib, ops  # noqa: F401
from ._lib import is_deterministic, set_deterministic  # noqa: F401
from .registry import BACKBONES, HEADS, LOSSES, MODELS, SEGMENTORS, register_into_mmseg  # noqa: F401
from .lednet import LEDNet
from .led_head import LEDHead
from .losses import (CrossEntropyLoss, DiceLoss, FocalLoss, HuasdorffDisstanceLoss, LovaszLoss,  # noqa: F401
                     OhemCrossEntropy, TverskyLoss)
from .segmentor import EncoderDecoder, SegDataPreProcessor, SegDataSample, SegTTAModel  # noqa: F401
from .config import load_config  # noqa: F401
from .train import Trainer  # noqa: F401
from .metrics import IoUMetric  # noqa: F401
from .checkpoint import init_model, load_checkpoint, resume, save_checkpoint  # noqa: F401
from . import transforms  # noqa: F401

MODELS.register_module(module=LEDNet)
MODELS.register_module(module=LEDHead)

__all__ = ['MODELS', 'LEDNet', 'LEDHead', 'OhemCrossEntropy', 'CrossEntropyLoss', 'DiceLoss', 'FocalLoss',
           'TverskyLoss', 'LovaszLoss', 'HuasdorffDisstanceLoss', 'EncoderDecoder', 'SegTTAModel', 'SegDataSample',
           'load_config', 'ops', 'register_into_mmseg', 'Trainer']
