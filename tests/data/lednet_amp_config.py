# tests/data/lednet_test_config.py under mmengine's AmpOptimWrapper: the optimizer moves into the wrapper section, and the
# wrapper's type switches on the step guard (a step whose gradient holds an Inf or a NaN is left out)
_base_ = ['./lednet_test_config.py']
optim_wrapper = dict(type='AmpOptimWrapper', optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005),
                     loss_scale='dynamic')
