# the test config (lednet_test_config.py) with the head's two losses replaced: CrossEntropyLoss on the context logits,
# LovaszLoss (the surrogate of the reported IoU) on the spatial logits
_base_ = './lednet_test_config.py'
model = dict(decode_head=dict(loss_decode=[
    dict(type='CrossEntropyLoss', avg_non_ignore=True),
    dict(type='LovaszLoss', reduction='none', loss_weight=0.4)]))
