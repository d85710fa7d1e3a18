# tests/data/lednet_test_config.py with mmengine's EMAHook switched on (momentum chosen large: three iterations must
# move the average visibly)
_base_ = ['./lednet_test_config.py']
custom_hooks = [dict(type='EMAHook', momentum=0.1)]
