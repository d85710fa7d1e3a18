"""Gradient clipping (optim_wrapper.clip_grad) fused into the SGD step: the norm pass over the flat gradient buffer, the
clipping SGD launch, the Trainer around them, the config / command-line path and the C ABI's argument checks.
Expected values come from torch itself (torch.nn.utils.clip_grad_norm_ / clip_grad_value_ + torch.optim.SGD), which is
what mmengine's OptimWrapper._clip_grad calls.  Emulator on the CPU; the same bodies on the MI355X with -m gpu."""
import copy
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from conftest import slow_on_emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'tests', 'data', 'lednet_test_config.py')
_DEV = [torch.device('cpu')]


@pytest.fixture(autouse=True)
def _track_device(request):
    _DEV[0] = request.getfixturevalue('be').dev if 'be' in request.fixturenames else torch.device('cpu')
    yield


def D(t):
    return t.to(_DEV[0])


def _norm_type(name):
    from led_net_amd import _lib
    return {'l2': _lib.NORM_L2, 'inf': _lib.NORM_INF}[name]


def _total(flat, name):
    """grad_norm_partials + the host-side combine of the partials -> (total as a 0-dim f32 tensor on the CPU, partials)"""
    from led_net_amd import ops_train as T
    part = torch.full((T.norm_partials_count(flat.numel()),), -7.0, device=flat.device)    # (every slot must be written)
    T.grad_norm_partials(flat, _norm_type(name), part)
    part = part.cpu()
    if name == 'l2':
        return part.double().sum().sqrt().float(), part
    return part.max(), part             # torch.max propagates NaN


# --------------------------------------------------------------------------- #
# 1. the norm pass
# --------------------------------------------------------------------------- #
# (length, offset in floats from a 16-byte aligned address)
NORM_CASES = [(1, 0), (1, 1), (2, 3), (3, 0), (5, 1), (7, 2), (1023, 0), (4097, 1), (65537, 3), (1_500_003, 0),
              (1_572_864, 1), (2_100_001, 2)]


@pytest.mark.parametrize('n,off', NORM_CASES)
@pytest.mark.parametrize('name', ['l2', 'inf'])
def test_norm_pass(be, name, n, off):
    from led_net_amd import ops_train as T
    g = torch.Generator().manual_seed(n + off)
    base = D(torch.randn(n + 8, generator=g))
    assert base.data_ptr() % 16 == 0
    flat = base[off:off + n]
    assert flat.data_ptr() % 16 == 4 * off
    got, part = _total(flat, name)
    if n >= 1_500_000:
        assert part.numel() == 256 and bool((part > 0).all())        # all 256 workgroups had elements
    ref = flat.cpu()
    if name == 'l2':
        want = ref.double().norm()
        print(f'{name} n={n} off={off}: rel err {abs(float(got) - float(want)) / float(want):.3e}')
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=0)
    else:
        assert float(got) == float(ref.abs().max())                   # exactly
    # bit-reproducible, deterministic mode off: no atomics, one combining order
    from led_net_amd import _lib
    assert not _lib.is_deterministic()
    again = _total(flat, name)[1]
    assert torch.equal(part.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize('name', ['l2', 'inf'])
@pytest.mark.parametrize('n,pos', [(1, 0), (6, 5), (4099, 0), (4099, 4098), (300_001, 123_457), (1_500_003, 1_499_999)])
def test_norm_pass_propagates_nan(be, name, n, pos):
    flat = torch.randn(n + 1)[1:]                    # (one float off 16-byte alignment: head, vectors and tail all in use)
    flat[pos] = float('nan')
    got, _ = _total(D(flat.clone()).contiguous(), name)
    assert math.isnan(float(got))
    got, _ = _total(D(torch.cat([torch.zeros(1), flat]))[1:], name)
    assert math.isnan(float(got))


@pytest.mark.parametrize('name', ['l2', 'inf'])
def test_all_zero_gradient_gives_zero_norm_and_coef_one(be, name):
    from led_net_amd import ops_train as T
    p = D(torch.randn(5000))
    g, m = torch.zeros_like(p), torch.zeros_like(p)
    p0 = p.clone()
    tab = T.SgdTable([p], [g], [m])
    clip = T.GradClip(p.device, g.numel(), norm_type=_norm_type(name), max_norm=1.0)
    clip.norm_pass(g)
    tab.step(0.01, 0.9, 0.0, clip=clip)
    assert float(clip.total_norm) == 0.0 and float(clip.coef) == 1.0
    assert torch.equal(p, p0)                        # zero gradient, no weight decay: nothing moves


# --------------------------------------------------------------------------- #
# 2. the clipping SGD launch (the shapes of test_ops_bwd.test_sgd_step, gradients as views of ONE flat buffer)
# --------------------------------------------------------------------------- #
SHAPES = ((5,), (3, 4), (1000,), (7, 3, 3, 3))


def _flat_views(shapes, dev):
    n = sum(math.prod(s) for s in shapes)
    flat = torch.zeros(n + 3, device=dev)[3:]        # (not 16-byte aligned, as a slice of a larger buffer may be)
    views, off = [], 0
    for s in shapes:
        k = math.prod(s)
        views.append(flat[off:off + k].view(s))
        off += k
    return flat, views


def _clip_sgd_case(mode, grad_scale):
    """three steps with gradients growing 1x, 2x, 3x; mode 'l2' / 'inf': max_norm = 1.5 x the (scaled) norm of the first
    step's gradient, so step 1 passes unclipped and steps 2 and 3 are clipped; 'value': clip_value 0.8 / grad_scale'd"""
    from led_net_amd import _lib, ops_train as T
    torch.manual_seed(1)
    ps = [torch.randn(s) for s in SHAPES]
    gs = [torch.randn_like(p) for p in ps]
    ref = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.SGD(ref, lr=0.01, momentum=0.9, weight_decay=5e-4)
    pd = [D(p.clone()) for p in ps]
    flat, gd = _flat_views(SHAPES, _DEV[0])
    md = [torch.zeros_like(p) for p in pd]
    tab = T.SgdTable(pd, gd, md)
    if mode == 'value':
        clip = T.GradClip(_DEV[0], flat.numel(), norm_type=_lib.NORM_NONE, clip_value=0.8)
    else:
        p_ = 2.0 if mode == 'l2' else math.inf
        first = float(torch.linalg.vector_norm(torch.cat([g.reshape(-1) for g in gs]) * grad_scale, p_))
        max_norm = 1.5 * first
        clip = T.GradClip(_DEV[0], flat.numel(), norm_type=_norm_type(mode), max_norm=max_norm)
    coefs = []
    for it in range(3):
        for r_, g in zip(ref, gs):
            r_.grad = g.clone() * (it + 1) * grad_scale          # the gradient the update uses (DDP's mean)
        if mode == 'value':
            torch.nn.utils.clip_grad_value_(ref, 0.8)
        else:
            want_norm = torch.nn.utils.clip_grad_norm_(ref, max_norm, norm_type=p_)
        opt.step()
        for g, g0 in zip(gd, gs):
            g.copy_(D(g0 * (it + 1)))
        clip.norm_pass(flat)
        tab.step(0.01, 0.9, 5e-4, grad_scale, clip=clip)
        if mode != 'value':
            torch.testing.assert_close(clip.total_norm.cpu(), want_norm.float(), rtol=1e-5, atol=0)
            coefs.append(float(clip.coef))
        assert float(flat.abs().max()) == 0.0                    # gradients re-zeroed
    if mode != 'value':
        print('coef per step:', coefs)
        assert coefs[0] == 1.0 and coefs[1] < 1.0 and coefs[2] < coefs[1]
        torch.testing.assert_close(torch.tensor(coefs[1:]), torch.tensor([1.5 / 2, 1.5 / 3]), rtol=1e-5, atol=0)
    for p, r_ in zip(pd, ref):
        torch.testing.assert_close(p.cpu(), r_.detach(), rtol=1e-5, atol=1e-6)
    for m, r_ in zip(md, ref):
        torch.testing.assert_close(m.cpu(), opt.state[r_]['momentum_buffer'], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
@pytest.mark.parametrize('mode', ['l2', 'inf', 'value'])
def test_clip_sgd_step(be, mode, grad_scale):
    _clip_sgd_case(mode, grad_scale)


def test_clip_by_value_passes_nan_and_nonfinite_norm_is_not_masked(be):
    from led_net_amd import _lib, ops_train as T
    # by value: torch.clamp keeps a NaN gradient, the others are clamped
    p = D(torch.zeros(8))
    flat, (g,) = _flat_views(((8,),), _DEV[0])
    g.copy_(D(torch.tensor([float('nan'), 5.0, -5.0, 0.25, 0, 0, 0, 0])))
    want = torch.clamp(g.cpu(), -1.0, 1.0)
    m = torch.zeros_like(p)
    T.SgdTable([p], [g], [m]).step(1.0, 0.0, 0.0, clip=T.GradClip(_DEV[0], 8, norm_type=_lib.NORM_NONE, clip_value=1.0))
    torch.testing.assert_close(p.cpu(), -want, rtol=0, atol=0, equal_nan=True)
    assert math.isnan(float(p[0])) and float(p[1]) == -1.0 and float(p[2]) == 1.0 and float(p[3]) == -0.25
    # by norm, error_if_nonfinite=False: the coefficient is NaN and so is every parameter
    for bad, name in ((float('nan'), 'l2'), (float('nan'), 'inf'), (float('inf'), 'l2')):
        p = D(torch.ones(8))
        g.copy_(D(torch.tensor([bad, 1.0, 0, 0, 0, 0, 0, 0])))
        ref = torch.ones(8, requires_grad=True)
        ref.grad = g.cpu().clone()
        torch.nn.utils.clip_grad_norm_([ref], 1.0, norm_type=2.0 if name == 'l2' else math.inf)
        torch.optim.SGD([ref], lr=1.0).step()
        clip = T.GradClip(_DEV[0], 8, norm_type=_norm_type(name), max_norm=1.0)
        clip.norm_pass(flat)
        T.SgdTable([p], [g], [torch.zeros_like(p)]).step(1.0, 0.0, 0.0, clip=clip)
        assert torch.equal(torch.isnan(p.cpu()), torch.isnan(ref.detach())), (bad, name, p, ref)
        torch.testing.assert_close(p.cpu(), ref.detach(), rtol=1e-6, atol=0, equal_nan=True)


# --------------------------------------------------------------------------- #
# 3. a neutral clip is free: coef == 1 gives the bits of ledn_sgd_step
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('name', ['l2', 'inf'])
def test_neutral_clip_is_bit_identical_to_plain_sgd(be, name):
    from led_net_amd import ops_train as T
    torch.manual_seed(2)
    shapes = SHAPES + ((70000,),)
    ps = [torch.randn(s) for s in shapes]
    gs = [torch.randn(s) for s in shapes]
    res = []
    for clipped in (False, True):
        pd = [D(p.clone()) for p in ps]
        flat, gd = _flat_views(shapes, _DEV[0])
        md = [torch.zeros_like(p) for p in pd]
        tab = T.SgdTable(pd, gd, md)
        clip = T.GradClip(_DEV[0], flat.numel(), norm_type=_norm_type(name), max_norm=1e30) if clipped else None
        for it in range(2):
            for g, g0 in zip(gd, gs):
                g.copy_(D(g0 * (it + 1)))
            if clip is not None:
                clip.norm_pass(flat)
            tab.step(0.01, 0.9, 5e-4, 0.5, clip=clip)
        if clip is not None:
            assert float(clip.coef) == 1.0
        res.append(([p.cpu() for p in pd], [m.cpu() for m in md]))
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# --------------------------------------------------------------------------- #
# 4. the whole step
# --------------------------------------------------------------------------- #
def _small_trainer(dev, seed=304, batch=2, **kw):
    import led_net_amd as L
    torch.manual_seed(seed)
    cfg = L.load_config(CFG)
    for c in cfg['model']['decode_head']['loss_decode']:
        c['min_kept'] = 20000
    model = L.MODELS.build(cfg['model']).to(dev)
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (batch, 3, 320, 320), dtype=torch.uint8, generator=g).to(dev)
    lab = torch.randint(0, 2, (batch, 1, 320, 320), dtype=torch.int64, generator=g)
    lab[:, :, :6, :] = 255
    samples = [L.SegDataSample(gt=lab[i].to(dev)) for i in range(batch)]
    return L.Trainer(model, cfg, max_iters=1000, **kw), model, cfg, img, samples


def _torch_clip_sgd(tr, params, grads, moms, clip_grad, lr):
    """torch's clip + SGD over the trainer's live tensors (host copies) -> (updated parameters, total norm)"""
    ref = [p.clone().requires_grad_(True) for p in params]
    for r_, g in zip(ref, grads):
        r_.grad = g.clone()
    opt = torch.optim.SGD(ref, lr=lr, momentum=tr.momentum, weight_decay=tr.wd)
    for r_, m in zip(ref, moms):
        opt.state[r_]['momentum_buffer'] = m.clone()
    norm = torch.nn.utils.clip_grad_norm_(ref, clip_grad['max_norm'], norm_type=float(clip_grad.get('norm_type', 2)))
    opt.step()
    return [r_.detach() for r_ in ref], norm


def _whole_step_case(dev, norm_type):
    import led_net_amd as L
    tr, model, cfg, img, samples = _small_trainer(dev)
    out = tr.train_step(img, samples)                       # no clipping: attaches the flat gradient views / sinks
    assert 'grad_norm' not in out and tr._sink_map
    state = {k: v.clone() for k, v in model.state_dict().items()}
    tr.forward_backward(img, samples)
    live = [i for i, p in enumerate(tr.params) if any(p is q for q in tr.live)]
    grads = [tr.views[i].detach().cpu().clone() for i in live]
    flat = tr.flat_grad.detach().cpu().clone()
    assert flat.numel() > sum(g.numel() for g in grads)     # (parameters without gradient: zeros in the buffer ...)
    assert int((flat != 0).sum()) == sum(int((g != 0).sum()) for g in grads) > 0
    model.load_state_dict(state)                            # the running statistics moved in that forward
    params = [tr.params[i].detach().cpu().clone() for i in live]
    moms = [tr.moms[i].detach().cpu().clone() for i in live]
    p_ = 2.0 if norm_type == 2 else math.inf
    measured = float(torch.linalg.vector_norm(flat.double(), p_))
    assert math.isfinite(measured) and measured > 0
    clip_grad = dict(max_norm=0.5 * measured, norm_type=norm_type)
    tr.flat_grad.zero_()
    tr.set_clip_grad(clip_grad)
    lr = tr.lr()
    out = tr.train_step(img, samples)
    coef, got_norm = float(tr.clip.coef), out['grad_norm'].cpu()
    want, want_norm = _torch_clip_sgd(tr, params, grads, moms, clip_grad, lr)
    print(f'norm_type {norm_type}: grad_norm {float(got_norm):.6g} (torch {float(want_norm):.6g}), coef {coef:.6g}')
    assert got_norm.dim() == 0 and coef < 1.0
    torch.testing.assert_close(got_norm, want_norm.float(), rtol=1e-5, atol=0)
    torch.testing.assert_close(torch.tensor(coef), (clip_grad['max_norm'] / (want_norm + 1e-6)).float(), rtol=1e-5, atol=0)
    for i, w in zip(live, want):
        torch.testing.assert_close(tr.params[i].detach().cpu(), w, rtol=1e-5, atol=1e-6)
    assert float(tr.flat_grad.abs().max()) == 0.0


def test_whole_step_with_clipping_vs_torch(emu):
    _whole_step_case(torch.device('cpu'), 2)


def test_whole_step_with_inf_norm_clipping_vs_torch(emu):
    slow_on_emu(torch.device('cpu'))
    _whole_step_case(torch.device('cpu'), 'inf')


@pytest.mark.gpu
@pytest.mark.parametrize('norm_type', [2, 'inf'])
def test_whole_step_with_clipping_vs_torch_gpu(norm_type):
    import led_net_amd as L
    L.set_deterministic(True)           # the gradients of the two passes are then the same bits
    try:
        _whole_step_case(torch.device('cuda:0'), norm_type)
    finally:
        L.set_deterministic(False)


# --------------------------------------------------------------------------- #
# 5. the captured graph
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
def test_captured_step_with_clipping_equals_eager():
    import led_net_amd as L
    dev = torch.device('cuda:0')
    L.set_deterministic(True)
    try:
        def batches(n):
            g = torch.Generator().manual_seed(23)
            out = []
            for _ in range(n):
                img = torch.randint(0, 256, (2, 3, 320, 320), dtype=torch.uint8, generator=g).to(dev)
                lab = torch.randint(0, 2, (2, 1, 320, 320), dtype=torch.int64, generator=g)
                lab[:, :, :6, :] = 255
                out.append((img, [L.SegDataSample(gt=lab[i].to(dev)) for i in range(2)]))
            return out
        bs = batches(2)
        # the clip must engage: half of the first batch's gradient norm, measured with a neutral clip
        tr, model, cfg, img, samples = _small_trainer(dev, clip_grad=dict(max_norm=1e30))
        init = copy.deepcopy(model.state_dict())
        m = 0.5 * float(tr.train_step(*bs[0])['grad_norm'])
        assert math.isfinite(m) and m > 0

        def run(graph):
            tr, model, _, _, _ = _small_trainer(dev, clip_grad=dict(max_norm=m))
            model.load_state_dict(init)
            outs = []
            if graph:
                tr.capture(*bs[0], warmup=2, restore=True)
                for b in bs:
                    o = tr.replay(*b)
                    assert o is tr._static_out
                    outs.append(({k: v.detach().clone() for k, v in o.items()}, float(tr.clip.coef)))
            else:
                snap = ([p.detach().clone() for p in tr.params], [b_.detach().clone() for b_ in model.buffers()], tr.iter)
                for _ in range(2):
                    tr.train_step(*bs[0])
                with torch.no_grad():
                    for p, v in zip(tr.params, snap[0]):
                        p.copy_(v)
                    for b_, v in zip(model.buffers(), snap[1]):
                        b_.copy_(v)
                    tr.flat_mom.zero_()
                tr.iter = snap[2]
                for b in bs:
                    o = tr.train_step(*b)
                    outs.append(({k: v.detach().clone() for k, v in o.items()}, float(tr.clip.coef)))
            torch.cuda.synchronize()
            return outs, {k: v.detach().clone() for k, v in model.state_dict().items()}, tr.flat_mom.clone()
        eager, graph = run(False), run(True)
        norms = [float(o['grad_norm']) for o, _ in graph[0]]
        print('grad_norm per replay:', norms, 'coef:', [c for _, c in graph[0]], 'max_norm', m)
        assert norms[0] != norms[1]                          # _static_out shows the value of each replay
        assert graph[0][0][1] < 1.0                          # clipping engaged
        for i, ((a, ca), (b, cb)) in enumerate(zip(eager[0], graph[0])):
            assert ca == cb
            for k in a:
                assert torch.equal(a[k], b[k]), (i, k, a[k], b[k])
        bad = [k for k in eager[1] if not torch.equal(eager[1][k], graph[1][k])]
        assert not bad, bad[:5]
        assert torch.equal(eager[2], graph[2])
    finally:
        L.set_deterministic(False)


# --------------------------------------------------------------------------- #
# 6. two ranks (gloo, emulator): the pattern of tests/test_distributed.py's world-2 = world-1 test
# --------------------------------------------------------------------------- #
CLIP_W2 = dict(max_norm=0.05)       # (far below this random-init step's gradient norm: asserted through coef < 1)


def _w2_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['LEDN_EXPERIMENTAL'] = '1'
    os.environ['LEDN_MULTI_COMM'] = '1'
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import led_net_amd as L
    from conftest import bind_emu
    import test_distributed as TD
    cfg = TD._cmp_cfg()
    img, lab = TD._cmp_batch()
    per = img.shape[0] // world
    img, lab = img[rank * per:(rank + 1) * per], lab[rank * per:(rank + 1) * per]
    with bind_emu():
        model = L.MODELS.build(cfg['model'])
        model.load_state_dict(torch.load(os.path.join(out_dir, 'init.pt')))
        tr = L.Trainer(model, cfg, world_size=world, clip_grad=CLIP_W2)
        TD._two_steps(tr, img, [L.SegDataSample(gt=lab[i]) for i in range(per)])
    torch.save({'sd': {k: v.detach().clone() for k, v in model.state_dict().items()},
                'norm': tr.clip.total_norm.clone(), 'coef': tr.clip.coef.clone()}, os.path.join(out_dir, f'w2_{rank}.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(1500)
def test_world2_with_clipping_equals_world1_on_concatenated_batch(tmp_path):
    """as test_distributed.test_ddp_world2_equals_world1_on_concatenated_batch (same configuration, batch, two-step
    protocol and tolerance: median < 3 %, worst < 25 % of the update norm), with clip_grad on: the norm is that of the
    AVERAGED gradient, bit-equal on both ranks, and equals the single-process norm on the concatenated batch"""
    sys.path.insert(0, ROOT)
    import led_net_amd as L
    from conftest import bind_emu
    import test_distributed as TD
    cfg = TD._cmp_cfg()
    torch.manual_seed(100)
    img, lab = TD._cmp_batch()
    with bind_emu():
        model = L.MODELS.build(cfg['model'])
        init = {k: v.detach().clone() for k, v in model.state_dict().items()}
        torch.save(init, tmp_path / 'init.pt')
        port = 35500 + (os.getpid() % 2000)
        ctx = mp.spawn(_w2_worker, args=(2, port, str(tmp_path)), nprocs=2, join=False)
        tr = L.Trainer(model, cfg, world_size=1, clip_grad=CLIP_W2)
        TD._two_steps(tr, img, [L.SegDataSample(gt=lab[i]) for i in range(4)])
    while not ctx.join():
        pass
    one = model.state_dict()
    r0, r1 = torch.load(tmp_path / 'w2_0.pt'), torch.load(tmp_path / 'w2_1.pt')
    print('grad_norm world 1', float(tr.clip.total_norm), 'world 2', float(r0['norm']), float(r1['norm']),
          'coef', float(tr.clip.coef), float(r0['coef']))
    assert torch.equal(r0['norm'], r1['norm']) and torch.equal(r0['coef'], r1['coef'])
    assert float(r0['coef']) < 1.0 and float(tr.clip.coef) < 1.0
    assert abs(float(r0['norm']) - float(tr.clip.total_norm)) < 3e-2 * float(tr.clip.total_norm)
    for k in r0['sd']:
        assert torch.equal(r0['sd'][k], r1['sd'][k]), k
    two = r0['sd']
    rels = []
    for k, v in one.items():
        if not v.is_floating_point() or 'running_' in k:
            continue
        upd = (v - init[k]).norm().item()
        if upd < 1e-6:
            continue
        rels.append(((two[k] - v).norm().item() / upd, k))
    rels.sort(reverse=True)
    assert len(rels) > 100
    assert rels[len(rels) // 2][0] < 3e-2 and rels[0][0] < 0.25, (rels[len(rels) // 2], rels[:5])


# --------------------------------------------------------------------------- #
# 7. configuration
# --------------------------------------------------------------------------- #
def _tiny_model():
    import led_net_amd as L
    return L.MODELS.build(L.load_config(CFG)['model']), L.load_config(CFG)


def test_clip_grad_is_read_from_optim_wrapper_and_the_argument_wins():
    import led_net_amd as L
    from led_net_amd import _lib
    model, cfg = _tiny_model()
    assert 'optim_wrapper' not in cfg
    assert L.Trainer(model, cfg).clip is None
    cfg['optim_wrapper'] = dict(type='OptimWrapper', optimizer=cfg['optimizer'], clip_grad=None)
    assert L.Trainer(model, cfg).clip is None
    cfg['optim_wrapper']['clip_grad'] = dict(max_norm=3.0, norm_type='inf')
    tr = L.Trainer(model, cfg)
    assert (tr.clip.norm_type, tr.clip.max_norm) == (_lib.NORM_INF, 3.0)
    assert (tr.base_lr, tr.momentum, tr.wd) == (0.01, 0.9, 5e-4)          # still cfg['optimizer']
    tr = L.Trainer(model, cfg, clip_grad=dict(type='norm', max_norm=0.5, norm_type=2.0))
    assert (tr.clip.norm_type, tr.clip.max_norm) == (_lib.NORM_L2, 0.5)
    tr = L.Trainer(model, cfg, clip_grad=dict(type='value', clip_value=0.1))
    assert (tr.clip.norm_type, tr.clip.clip_value) == (_lib.NORM_NONE, 0.1)
    for nt, want in ((2, _lib.NORM_L2), (2.0, _lib.NORM_L2), ('inf', _lib.NORM_INF), (float('inf'), _lib.NORM_INF)):
        assert L.Trainer(model, clip_grad=dict(max_norm=1, norm_type=nt)).clip.norm_type == want
    n = tr.flat_grad.numel()
    tr = L.Trainer(model, clip_grad=dict(max_norm=1.0))
    assert tr.clip.buf.numel() == tr.clip.n_partials + 2 == min(256, -(-n // 4096)) + 2     # [partials | total_norm | coef]
    assert tr.clip.total_norm.dim() == 0 and tr.clip.total_norm.data_ptr() == tr.clip.buf[-2:].data_ptr()


@pytest.mark.parametrize('bad,word', [
    (dict(max_norm=1.0, norm_type=1), 'norm_type'), (dict(max_norm=1.0, norm_type='l2'), 'norm_type'),
    (dict(max_norm=1.0, norm_type=3.0), 'norm_type'), (dict(max_norm=0.0), 'max_norm'), (dict(max_norm=-1.0), 'max_norm'),
    (dict(max_norm=float('nan')), 'max_norm'), (dict(norm_type=2), 'max_norm'), (dict(max_norm=1.0, max_nrom=2.0), 'max_nrom'),
    (dict(type='norms', max_norm=1.0), 'type'), (dict(type='value'), 'clip_value'), (dict(type='value', clip_value=0), 'clip_value'),
    (dict(type='value', clip_value=1.0, max_norm=1.0), 'max_norm'), (dict(max_norm=1.0, error_if_nonfinite=True), 'error_if_nonfinite'),
    (1.0, 'dict')])
def test_bad_clip_grad_raises_value_error(bad, word):
    import led_net_amd as L
    model, cfg = _tiny_model()
    with pytest.raises(ValueError, match=word):
        L.Trainer(model, clip_grad=bad)
    cfg['optim_wrapper'] = dict(clip_grad=bad)
    with pytest.raises(ValueError, match=word):
        L.Trainer(model, cfg)
    if isinstance(bad, dict) and bad.get('error_if_nonfinite'):
        with pytest.raises(ValueError, match='not supported'):
            L.Trainer(model, clip_grad=bad)


def test_returned_keys_by_value_and_off(emu):
    """grad_norm only with clipping by norm (mmengine logs none for clip by value); with clipping off the step returns
    exactly the keys the model's loss dict has"""
    dev = torch.device('cpu')
    tr, model, cfg, img, samples = _small_trainer(dev, batch=1, clip_grad=dict(type='value', clip_value=1e-4))
    init = {k: v.clone() for k, v in model.state_dict().items()}
    lr = tr.lr()
    out = tr.train_step(img, samples)
    assert sorted(out) == ['decode.acc_seg', 'decode.loss_context', 'decode.loss_spatial']
    # every gradient element clamped to +-1e-4, no momentum history: |update| <= lr * (1e-4 + wd * |p|), plus the
    # rounding of the f32 subtraction p - lr * m (half an ulp of |p|; two allowed for the update's own roundings)
    eps = torch.finfo(torch.float32).eps
    worst = 0.0
    for k, v in model.state_dict().items():
        if v.is_floating_point() and 'running_' not in k:
            bound = lr * (1e-4 + tr.wd * init[k].abs()) * (1 + 1e-5) + 2 * eps * init[k].abs() + 1e-12
            assert bool(((v - init[k]).abs() <= bound).all()), k
            worst = max(worst, float((v - init[k]).abs().max()))
    assert worst > 0.5 * lr * 1e-4                         # ... and the clamp was reached
    tr.set_clip_grad(None)
    assert tr.clip is None
    tr.set_clip_grad(dict(max_norm=2.0))
    assert tr.clip.max_norm == 2.0


@pytest.mark.gpu
def test_train_cli_takes_clip_grad_from_cfg_options(tmp_path):
    def run(extra, wd):
        env = dict(os.environ, PYTHONPATH=ROOT, LEDN_DETERMINISTIC='1')
        args = [sys.executable, 'tools/train.py', CFG, '--max-iters', '3', '--batch-size', '2', '--height', '320',
                '--width', '320', '--f32', '--work-dir', str(tmp_path / wd)] + extra
        r = subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, f'{args}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
        line = [ln for ln in r.stdout.splitlines() if re.search(r'\[\s*3/3\]', ln)]
        assert line, r.stdout[-2000:]
        return line[0]
    plain = run([], 'plain')
    assert 'grad_norm' not in plain
    clipped = run(['--cfg-options', "optim_wrapper.clip_grad={'max_norm': 0.01}"], 'clipped')
    dotted = run(['--cfg-options', 'optim_wrapper.clip_grad.max_norm=0.01'], 'dotted')
    print(plain, clipped, dotted, sep='\n')
    m = re.search(r'grad_norm: ([0-9.eE+-]+|nan|inf)', clipped)
    assert m and math.isfinite(float(m.group(1))) and float(m.group(1)) > 0
    loss = [re.search(r'loss_context: ([0-9.eE+-]+)', ln).group(1) for ln in (plain, clipped, dotted)]
    assert loss[1] == loss[2] and loss[1] != loss[0]       # both spellings reach the trainer, and the clip changes the run


# --------------------------------------------------------------------------- #
# 8. argument errors of the C entry points
# --------------------------------------------------------------------------- #
def test_entry_points_reject_bad_arguments(emu):
    from led_net_amd import _lib, ops_train as T
    lib = _lib.get_lib().cdll
    g = torch.randn(100)
    part = torch.zeros(256 + 2)
    gp, pp = g.data_ptr(), part.data_ptr()
    assert lib.ledn_grad_norm_partials(gp, 100, _lib.NORM_L2, pp, 1, None) == _lib.OK
    assert lib.ledn_grad_norm_partials(gp, 100, _lib.NORM_INF, pp, 256, None) == _lib.OK
    for n_part in (0, -1, 257):
        assert lib.ledn_grad_norm_partials(gp, 100, _lib.NORM_L2, pp, n_part, None) == _lib.EINVAL
    for nt in (_lib.NORM_NONE, 1, 3, -2):
        assert lib.ledn_grad_norm_partials(gp, 100, nt, pp, 1, None) == _lib.EINVAL
    assert lib.ledn_grad_norm_partials(None, 100, _lib.NORM_L2, pp, 1, None) == _lib.EINVAL
    assert lib.ledn_grad_norm_partials(gp, 100, _lib.NORM_L2, None, 1, None) == _lib.EINVAL
    assert lib.ledn_grad_norm_partials(gp, 0, _lib.NORM_L2, pp, 1, None) == _lib.EINVAL
    p, m = torch.randn(100), torch.zeros(100)
    tab = T.SgdTable([p], [g], [m])

    def step(n_part, nt, max_norm, clip_value, partials=pp):
        return lib.ledn_sgd_step_clip(tab.table.data_ptr(), 1, 100, 0.01, None, 0.9, 5e-4, 1.0, partials, n_part, nt,
                                      max_norm, clip_value, pp + 4 * 256, None)
    p0 = p.clone()
    for n_part in (0, -1, 257):
        assert step(n_part, _lib.NORM_L2, 1.0, 0.0) == _lib.EINVAL
    for nt in (1, 3, -2):
        assert step(1, nt, 1.0, 0.0) == _lib.EINVAL
    for mx in (0.0, -1.0, float('nan')):
        assert step(1, _lib.NORM_L2, mx, 0.0) == _lib.EINVAL
        assert step(1, _lib.NORM_INF, mx, 0.0) == _lib.EINVAL
    assert step(1, _lib.NORM_L2, 1.0, 0.0, partials=None) == _lib.EINVAL
    for cv in (0.0, -1.0, float('nan')):
        assert step(0, _lib.NORM_NONE, 0.0, cv) == _lib.EINVAL
    assert torch.equal(p, p0)                              # nothing was launched
    assert step(1, _lib.NORM_L2, 1.0, 0.0) == _lib.OK
    assert step(0, _lib.NORM_NONE, 0.0, 0.5, partials=None) == _lib.OK
    assert C.sizeof(_lib.SgdEntry) == 32
