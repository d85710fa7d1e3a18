# the test config (lednet_test_config.py) with the head's two losses replaced: CrossEntropyLoss on the context logits,
# HuasdorffDisstanceLoss (the boundary term: squared probability error weighted by squared pixel distances) on the
# spatial logits.  The term scales with squared pixel distances: on the 320 x 320 step of tests/test_hausdorff_step.py
# (filled shapes as labels, initial weights) it is 54 at loss_weight 1 against a cross-entropy of 4.1, so 0.1 puts the
# two terms at the same order (the step test asserts a ratio within [0.1, 10])
_base_ = './lednet_test_config.py'
model = dict(decode_head=dict(loss_decode=[
    dict(type='CrossEntropyLoss', avg_non_ignore=True),
    dict(type='HuasdorffDisstanceLoss', loss_weight=0.1)]))
