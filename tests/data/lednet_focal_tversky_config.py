# the test config (lednet_test_config.py) with the head's two losses replaced: FocalLoss on the context logits,
# TverskyLoss (false negatives weighted 0.7) on the spatial logits -- hard-pixel weighting without OHEM's selection
# next to the region loss usual for thin foreground
_base_ = './lednet_test_config.py'
model = dict(decode_head=dict(loss_decode=[
    dict(type='FocalLoss', gamma=2.0, alpha=0.5, loss_weight=1.0),
    dict(type='TverskyLoss', alpha=0.3, beta=0.7, loss_weight=0.4)]))
