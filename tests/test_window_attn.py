"""Window attention, forward and backward, at every kernel family the dispatchers can pick: generic head dim 8 / 16 /
32 x {f32, bf16} x {reflect-padded, tiling}, the matrix-core form (bf16, head dim 16, tiling), the backward's atomics
and partial-rows paths (more than 8 wavefronts per head, or deterministic mode) and the deterministic pad_out path --
against the attention expression in float64 on the CPU (bf16 operands rounded to bf16 first, then promoted).

Bounds, as the project states them for the same kernels (tests/test_ops_bwd.py):
  generic f32 forward    assert_close(rtol=1e-4, atol=1e-5)
  generic f32 backward   (1e-3, 1e-4)
  every bf16 form        rtol 2e-2 (forward) / 3e-2 (backward), atol 2e-2 * max|want|
The worst max|got - want| / max|want| per family is printed when the module finishes (pytest -s)."""
import contextlib
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
WS = 8
_WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    for (fam, dev), (err, what) in sorted(_WORST.items()):
        print(f'\n[worst] {fam:34s} {dev:4s} max|got-want|/max|want| {err:.3e}  at {what}', end='')
    print()


def gen(key, *shape):
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    return torch.randn(*shape, generator=g)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@contextlib.contextmanager
def deterministic(flag):
    from led_net_amd import _lib
    prev = _lib.is_deterministic()
    _lib.set_deterministic(flag)
    try:
        yield
    finally:
        _lib.set_deterministic(prev)


def attention(qkv, bias, heads):
    """qkv [n, 3C, H, W], bias [heads][query i][key j] -> [n, C, H, W]: reflect-extend to multiples of the window at the
    bottom / right, softmax(q k^T / sqrt(d) + bias) v per (window, head), crop"""
    n, c3, H, W = qkv.shape
    Cc, ws = c3 // 3, WS
    d = Cc // heads
    x = qkv
    if W % ws:
        x = F.pad(x, (0, ws - W % ws, 0, 0), mode='reflect')
    if H % ws:
        x = F.pad(x, (0, 0, 0, ws - H % ws), mode='reflect')
    Hp, Wp = x.shape[2:]
    hh, ww = Hp // ws, Wp // ws
    t = x.view(n, 3, heads, d, hh, ws, ww, ws).permute(1, 0, 4, 6, 2, 5, 7, 3).reshape(3, n * hh * ww, heads, 64, d)
    att = ((t[0] @ t[1].transpose(-2, -1)) * d ** -0.5 + bias.unsqueeze(0)).softmax(-1) @ t[2]
    return att.view(n, hh, ww, heads, ws, ws, d).permute(0, 3, 6, 1, 4, 2, 5).reshape(n, Cc, Hp, Wp)[:, :, :H, :W]


@functools.lru_cache(maxsize=None)
def case(n, H, W, heads, d, dt):
    """inputs (rounded to dt, in f32) and the f64 reference with its gradients; computed once, shared by both modes"""
    Cc = heads * d
    key = (n, H, W, heads, d)
    qkv = gen(('qkv',) + key, n, 3 * Cc, H, W).to(dt).float()
    bias = gen(('bias',) + key, heads, 64, 64) * 0.5
    dout = gen(('dout',) + key, n, Cc, H, W).to(dt).float()
    q64, b64 = qkv.double().requires_grad_(True), bias.double().requires_grad_(True)
    att = attention(q64, b64, heads)
    att.backward(dout.double())
    return qkv, bias, dout, att.detach(), q64.grad, b64.grad


def check(be, fam, got, want, rtol, atol, what):
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = float((got - want).abs().max() / want.abs().max())
    key = (fam, 'emu' if be.dev.type == 'cpu' else 'hip')
    if key not in _WORST or err > _WORST[key][0]:
        _WORST[key] = (err, what)
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda m: f'{fam} {what}: {m}')


MAPS = [(1, 8, 8), (1, 13, 11), (2, 24, 16), (3, 17, 24), (1, 5, 9), (2, 32, 40)]
HEADS_D = [(2, 16), (1, 32), (3, 8), (2, 32), (8, 16)]


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('heads,d', HEADS_D)
@pytest.mark.parametrize('n,H,W', MAPS)
def test_window_attn(be, n, H, W, heads, d, dt, det):
    from led_net_amd import ops, ops_train as T
    qkv, bias, dout, att, dqkv, dbias = case(n, H, W, heads, d, dt)
    bf = dt == BF16
    what = f'n{n} {H}x{W} heads{heads} d{d} {"bf16" if bf else "f32"} {"det" if det else "default"}'
    qd, dod = be(nhwc(qkv).to(dt)), be(nhwc(dout).to(dt))
    biasT = be(bias.permute(0, 2, 1).contiguous())
    with deterministic(det):
        got = ops.window_attn(qd, biasT, heads, WS)
        assert got.dtype == dt
        if bf:
            check(be, 'window_attn bf16', nchw(got), att, 2e-2, 2e-2 * float(att.abs().max()), what)
        else:
            check(be, 'window_attn f32', nchw(got), att, 1e-4, 1e-5, what)
        if d == 8:
            with pytest.raises(ops.LednError):
                T.window_attn_bwd(qd, biasT, dod, heads, WS)
            return
        gq, gbT = T.window_attn_bwd(qd, biasT, dod, heads, WS)
        assert gq.dtype == dt and gbT.dtype == F32
        gb = gbT.permute(0, 2, 1)
        if bf:
            check(be, 'window_attn_bwd bf16 dqkv', nchw(gq), dqkv, 3e-2, 2e-2 * float(dqkv.abs().max()), what)
            check(be, 'window_attn_bwd bf16 dbias', gb, dbias, 3e-2, 2e-2 * float(dbias.abs().max()), what)
        else:
            check(be, 'window_attn_bwd f32 dqkv', nchw(gq), dqkv, 1e-3, 1e-4, what)
            check(be, 'window_attn_bwd f32 dbias', gb, dbias, 1e-3, 1e-4, what)


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_window_attn_rejects_pad_not_smaller_than_map(be, dt):
    """H = 4: the reflect pad to 8 rows is 4, not smaller than the map"""
    from led_net_amd import ops, ops_train as T
    heads, Cc = 2, 32
    qkv = be(torch.zeros(1, 4, 8, 3 * Cc, dtype=dt))
    biasT = be(torch.zeros(heads, 64, 64))
    with pytest.raises(ops.LednError):
        ops.window_attn(qkv, biasT, heads, WS)
    with pytest.raises(ops.LednError):
        T.window_attn_bwd(qkv, biasT, be(torch.zeros(1, 4, 8, Cc, dtype=dt)), heads, WS)
