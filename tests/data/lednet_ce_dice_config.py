# the test config (lednet_test_config.py) with the head's two losses replaced: CrossEntropyLoss on the context logits,
# DiceLoss on the spatial logits -- the pair a two-class, few-percent-foreground task reaches for first
_base_ = './lednet_test_config.py'
model = dict(decode_head=dict(loss_decode=[
    dict(type='CrossEntropyLoss', avg_non_ignore=True, loss_weight=1.0),
    dict(type='DiceLoss', loss_weight=0.4)]))
