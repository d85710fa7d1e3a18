"""Resize, pooling, GETB mixing and relative-position-bias kernels, one case per instance the dispatchers can pick
(vector width x dtype pair x kernel family), against plain torch in float64 on the CPU.

Error measure: max|got - want| / max|want| over the whole tensor, want in f64.  bf16 operands are rounded to bf16 first
and then promoted to f64, so what is left is the kernel's own arithmetic and its one output rounding.

Bounds (none is tuned against the kernels):
  bf16 outputs                      2^-8   one rounding to an 8-bit significand: half an ulp (2^-8 of the binade's lower end) is at
                                           most 2^-8 / (1 + 2^-8) = 3.891e-3 of the value it rounds; the 1.5e-5 left under 2^-8 covers
                                           the f32 arithmetic before it (measured worst 3.861e-3: the bound has 1 % of headroom)
  f32 outputs of pools/GETB/relpos   1e-5   ~80 f32 ulp for sums of at most a few hundred terms
  f32 outputs of bilinear / adjoint  2^-23 * (16 + 3 * (H + W)), H x W the source map: the coordinate scale*(dst+0.5)-0.5 is at
                                           most the source size and is rounded once (contracted) or twice, so a lerp weight moves
                                           by up to 1.5 ulp of the coordinate and the output by that times 2*max|x| per axis

Every test loops over its maps inside one body (a few thousand elements per launch); the worst error per kernel family
is printed when the module finishes (pytest -s)."""
import contextlib
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
OPT_STREAM_FAST, STREAM_FAST_DEFAULT = 2, 91
TOL_BF16, TOL_F32 = 2.0 ** -8, 1e-5
PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)]
PAIR_IDS = ['f32-f32', 'bf16-bf16', 'bf16-f32', 'f32-bf16']
DT_IDS = {F32: 'f32', BF16: 'bf16'}

_WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    for (fam, dev), (err, bound, what) in sorted(_WORST.items()):
        print(f'\n[worst] {fam:28s} {dev:4s} err {err:.3e}  bound {bound:.3e}  at {what}', end='')
    print()


def gen(key, *shape):
    """seeded standard-normal f32 tensor; the seed is a digest of the case's key"""
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    return torch.randn(*shape, generator=g)


def q(t, dt):
    """values of t rounded to dt, kept in f32 (the reference promotes these to f64)"""
    return t.to(dt).float()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def rel_err(got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), 'non-finite output'
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def check(be, fam, got, want, bound, what):
    err = rel_err(got, want)
    key = (fam, 'emu' if be.dev.type == 'cpu' else 'hip')
    if key not in _WORST or err > _WORST[key][0]:
        _WORST[key] = (err, bound, what)
    assert err <= bound, f'{fam} {what}: max|got-want|/max|want| = {err:.3e} > {bound:.3e}'
    return err


def bil_bound(src):
    return 2.0 ** -23 * (16 + 3 * (src[0] + src[1]))


def out_bound(dt, f32_bound):
    return TOL_BF16 if dt == BF16 else f32_bound


@contextlib.contextmanager
def stream_fast_bit1_cleared():
    """LEDN_OPT_STREAM_FAST without bit 1: the general kernels instead of the wide / quad ones"""
    from led_net_amd import _lib
    lib = _lib.get_lib()
    lib.set_option(OPT_STREAM_FAST, STREAM_FAST_DEFAULT & ~2)
    try:
        yield
    finally:
        lib.set_option(OPT_STREAM_FAST, -1)


@contextlib.contextmanager
def deterministic(flag):
    from led_net_amd import _lib
    prev = _lib.is_deterministic()
    _lib.set_deterministic(flag)
    try:
        yield
    finally:
        _lib.set_deterministic(prev)


def raw_stream(t):
    from led_net_amd import _lib, ops
    return ops._stream(_lib.get_lib(), t)


# --------------------------------------------------------------------------- #
# 1. bilinear, NHWC: V in {4, 2, 1} x four dtype pairs, with and without add
# --------------------------------------------------------------------------- #
MAPS = [((9, 17), (18, 34)), ((9, 17), (35, 67)), ((8, 8), (3, 5)), ((1, 1), (4, 4)), ((3, 70), (6, 140)),
        ((4, 40), (9, 150)), ((2, 3), (1, 1)), ((16, 12), (7, 5)), ((5, 7), (5, 7))]
WIDE_MAPS = [((3, 70), (6, 140)), ((4, 40), (9, 150))]       # wider than 128: one vs two roundings of the coordinate differ


@functools.lru_cache(maxsize=None)
def _bilinear_case(src, dst, c, dx):
    x = q(gen(('bil', src, dst, c), 2, c, *src), dx)
    return x, F.interpolate(x.double(), size=dst, mode='bilinear', align_corners=False)


@pytest.mark.parametrize('dx,dy', PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize('c', [1, 2, 3, 4, 6, 12])
def test_bilinear_nhwc(be, c, dx, dy):
    from led_net_amd import ops
    for src, dst in MAPS:
        x, base = _bilinear_case(src, dst, c, dx)
        add = q(gen(('biladd', src, dst, c), 2, c, *dst), dy)
        for with_add in (False, True):
            want = base + add.double() if with_add else base
            got = ops.bilinear(be(nhwc(x).to(dx)), dst, add=be(nhwc(add).to(dy)) if with_add else None, out_dtype=dy)
            assert got.dtype == dy and tuple(got.shape) == (2, *dst, c)
            check(be, f'bilinear nhwc ->{DT_IDS[dy]}', nchw(got), want, out_bound(dy, bil_bound(src)),
                  f'{src}->{dst} C{c} x {DT_IDS[dx]} add={with_add}')


# --------------------------------------------------------------------------- #
# 2. bilinear, planar output + argmax
# --------------------------------------------------------------------------- #
PLANAR_C = [1, 2, 3, 4, 5, 8, 19]


@pytest.mark.parametrize('dx', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('c', PLANAR_C)
def test_bilinear_planar_argmax(be, c, dx):
    from led_net_amd import ops
    for src, dst in MAPS:
        x, base = _bilinear_case(src, dst, c, dx)
        add = gen(('planadd', src, dst, c), 2, c, *dst)
        for with_add in (False, True):
            want = base + add.double() if with_add else base
            got, am = ops.bilinear(be(nhwc(x).to(dx)), dst, add=be(nhwc(add)) if with_add else None, nchw=True, argmax=True)
            assert got.dtype == F32 and tuple(got.shape) == (2, c, *dst) and am.dtype == torch.uint8
            what = f'{src}->{dst} C{c} x {DT_IDS[dx]} add={with_add}'
            check(be, 'bilinear planar', got, want, bil_bound(src), what)
            first_max = np.argmax(got.cpu().numpy(), axis=1)          # numpy.argmax: the first maximum
            assert np.array_equal(am.cpu().numpy().astype(np.int64), first_max), what


@pytest.mark.parametrize('dx', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('c', [2, 3, 4, 5, 8, 19])
def test_bilinear_planar_argmax_tie(be, c, dx):
    """two classes' planes equal on the whole map and above the rest: the lower index wins"""
    from led_net_amd import ops
    src, dst = (9, 17), (35, 67)
    for a, b in {(0, 1), (c - 2, c - 1)}:
        x = gen(('tie', c, a), 2, c, *src)
        x[:, a] = x[:, b] = x[:, a].abs() + 10.0
        x = q(x, dx)
        got, am = ops.bilinear(be(nhwc(x).to(dx)), dst, nchw=True, argmax=True)
        assert torch.equal(got[:, a], got[:, b])
        assert bool((am == a).all()), (c, a, b, am.unique().tolist())


@pytest.mark.parametrize('c', [6, 7, 20])
def test_bilinear_planar_rejects_unsupported_c(be, c):
    from led_net_amd import ops
    with pytest.raises(ops.LednError):
        ops.bilinear(be(torch.zeros(1, 4, 4, c)), (8, 8), nchw=True, argmax=True)


# --------------------------------------------------------------------------- #
# 3. bilinear_bwd: wide, 2x V4/V2, general V4/V2/V1 x four dtype pairs
# --------------------------------------------------------------------------- #
BWD_MAPS = MAPS + [((4, 4), (32, 32)), ((2, 3), (9, 13)),      # >= 4x per axis: the wide kernel when C % 4 == 0
                   ((1, 3), (2, 6))]                           # exact 2x with H = 1


@functools.lru_cache(maxsize=None)
def _bilinear_bwd_case(src, dst, c, ddy):
    dy = q(gen(('bilbwd', src, dst, c), 2, c, *dst), ddy)
    x = torch.zeros(2, c, *src, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, size=dst, mode='bilinear', align_corners=False).backward(dy.double())
    return dy, x.grad


@pytest.mark.parametrize('ddy,ddx', PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize('c', [1, 2, 3, 4, 6, 12])
def test_bilinear_bwd(be, c, ddy, ddx):
    from led_net_amd import ops_train as T
    for src, dst in BWD_MAPS:
        dy, want = _bilinear_bwd_case(src, dst, c, ddy)
        got = T.bilinear_bwd(be(nhwc(dy).to(ddy)), src, out_dtype=ddx)
        assert got.dtype == ddx and tuple(got.shape) == (2, *src, c)
        check(be, f'bilinear_bwd ->{DT_IDS[ddx]}', nchw(got), want, out_bound(ddx, bil_bound(src)),
              f'{src}<-{dst} C{c} dy {DT_IDS[ddy]}')


@pytest.mark.parametrize('ddy,ddx', PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize('src,dst,c', [((4, 4), (32, 32), 4), ((2, 3), (9, 13), 12)])
def test_bilinear_bwd_general_instead_of_wide(be, src, dst, c, ddy, ddx):
    """LEDN_OPT_STREAM_FAST bit 1 cleared: bilinear_bwd_kernel<.., 4> on a shape that takes bilinear_bwd_wide_kernel by
    default; same candidates and weights, so on f32 the two agree to 1e-6 of max"""
    from led_net_amd import ops_train as T
    dy, want = _bilinear_bwd_case(src, dst, c, ddy)
    dyd = be(nhwc(dy).to(ddy))
    wide = T.bilinear_bwd(dyd, src, out_dtype=ddx)
    with stream_fast_bit1_cleared():
        general = T.bilinear_bwd(dyd, src, out_dtype=ddx)
    what = f'{src}<-{dst} C{c} dy {DT_IDS[ddy]} (general kernel)'
    check(be, f'bilinear_bwd ->{DT_IDS[ddx]}', nchw(general), want, out_bound(ddx, bil_bound(src)), what)
    if (ddy, ddx) == (F32, F32):
        assert rel_err(general, wide.cpu()) <= 1e-6, what


# --------------------------------------------------------------------------- #
# 4. adjointness of the product's own pair (no torch reference)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('src,dst', WIDE_MAPS + [((9, 17), (35, 67))])
def test_bilinear_pair_is_adjoint(be, src, dst):
    """<bilinear(x), dy> == <x, bilinear_bwd(dy)>, both formed in f64 from the returned f32 tensors.
    Bound: each element of y is off by at most B * max|y| (B = the bilinear bound of the map); summed against dy over
    numel(y) terms with errors of either sign that is B * sqrt(numel(y)) * max|y| * max|dy|.  The adjoint side's own
    error (numel(x) < numel(y) terms) is not added on top: the tighter figure is kept."""
    from led_net_amd import ops, ops_train as T
    c = 4
    x, dy = gen(('adjx', src, dst), 2, *src, c), gen(('adjdy', src, dst), 2, *dst, c)
    y = ops.bilinear(be(x), dst).cpu().double()
    dx = T.bilinear_bwd(be(dy), src).cpu().double()
    lhs, rhs = float((y * dy.double()).sum()), float((x.double() * dx).sum())
    tol = bil_bound(src) * y.numel() ** 0.5 * float(y.abs().max()) * float(dy.abs().max())
    print(f'adjointness {src}->{dst}: <y,dy> = {lhs:.9e}  <x,dx> = {rhs:.9e}  |diff| = {abs(lhs - rhs):.3e}  tol = {tol:.3e}')
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


# --------------------------------------------------------------------------- #
# 5. adaptive_avgpool
# --------------------------------------------------------------------------- #
AA_MAPS = [(19, 21), (5, 7), (1, 1), (16, 16), (33, 2), (40, 56)]     # (5, 7): windows overlap and H < S


@pytest.mark.parametrize('with_add', [False, True], ids=['plain', 'xadd'])
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('c', [1, 3, 8, 12, 20])                      # 12: 256 / (C/4) is not an integer
def test_adaptive_avgpool(be, c, dt, with_add):
    from led_net_amd import ops
    for hw in AA_MAPS:
        x = q(gen(('aa', hw, c), 2, c, *hw), dt)
        r = q(gen(('aar', hw, c), 2, c, *hw), dt)
        s64 = x.double() + r.double() if with_add else x.double()
        xd, rd = be(nhwc(x).to(dt)), be(nhwc(r).to(dt)) if with_add else None
        for S in (1, 2, 4, 8, 16):
            got = ops.adaptive_avgpool(xd, S, xadd=rd)
            assert got.dtype == F32
            check(be, 'adaptive_avgpool', nchw(got), F.adaptive_avg_pool2d(s64, S), TOL_F32, f'{hw} S{S} C{c} {DT_IDS[dt]}')


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_adaptive_avgpool_channel_limit(be, dt):
    """C / V == 256: every lane of the workgroup is a channel vector, one pixel lane; C = 1028 is one past it"""
    from led_net_amd import ops
    x = q(gen(('aalim',), 2, 1024, 3, 3), dt)
    got = ops.adaptive_avgpool(be(nhwc(x).to(dt)), 2)
    check(be, 'adaptive_avgpool', nchw(got), F.adaptive_avg_pool2d(x.double(), 2), TOL_F32, f'(3,3) S2 C1024 {DT_IDS[dt]}')
    with pytest.raises(ops.LednError):
        ops.adaptive_avgpool(be(torch.zeros(1, 3, 3, 1028, dtype=dt)), 2)


# --------------------------------------------------------------------------- #
# 6. avgpool3x3s2 and its adjoint
# --------------------------------------------------------------------------- #
P3_MAPS = [(19, 21), (2, 2), (1, 1), (16, 16), (1, 9), (2, 7)]


@functools.lru_cache(maxsize=None)
def _pool3_case(hw, c, dt):
    x = q(gen(('p3', hw, c), 2, c, *hw), dt)
    xr = x.double().requires_grad_(True)
    y = F.avg_pool2d(xr, 3, 2, 1)
    dy = q(gen(('p3dy', hw, c), *y.shape), dt)
    y.backward(dy.double())
    return x, y.detach(), dy, xr.grad


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('c', [1, 3, 8, 16, 24])    # bf16: C = 8, 16 take the quad adjoint, C = 24 (256 % 3 != 0) the element one
def test_avgpool3x3s2_and_adjoint(be, c, dt):
    from led_net_amd import ops, ops_train as T
    for hw in P3_MAPS:
        x, y, dy, dx = _pool3_case(hw, c, dt)
        what = f'{hw} C{c} {DT_IDS[dt]}'
        got = ops.avgpool3x3s2(be(nhwc(x).to(dt)))
        assert got.dtype == dt
        check(be, f'avgpool3x3s2 {DT_IDS[dt]}', nchw(got), y, out_bound(dt, TOL_F32), what)
        add = q(gen(('p3add', hw, c), 2, c, *hw), dt)
        for with_add in (False, True):
            gdx = T.avgpool3x3s2_bwd(be(nhwc(dy).to(dt)), hw, add=be(nhwc(add).to(dt)) if with_add else None)
            assert gdx.dtype == dt
            check(be, f'avgpool3x3s2_bwd {DT_IDS[dt]}', nchw(gdx), dx + add.double() if with_add else dx,
                  out_bound(dt, TOL_F32), f'{what} add={with_add}')


@pytest.mark.parametrize('c', [8, 16, 24])
def test_avgpool3x3s2_bwd_quad_equals_element_kernel(be, c):
    """the quad kernel keeps the element kernel's summation order: bit-identical on the same bf16 input"""
    from led_net_amd import ops_train as T
    for hw in P3_MAPS:
        _, _, dy, _ = _pool3_case(hw, c, BF16)
        add = be(nhwc(q(gen(('p3add', hw, c), 2, c, *hw), BF16)).bfloat16())
        dyd = be(nhwc(dy).bfloat16())
        for a in (None, add):
            quad = T.avgpool3x3s2_bwd(dyd, hw, add=a)
            with stream_fast_bit1_cleared():
                elem = T.avgpool3x3s2_bwd(dyd, hw, add=a)
            assert torch.equal(quad.view(torch.int16), elem.view(torch.int16)), (hw, c, a is not None)


# --------------------------------------------------------------------------- #
# 7. avgpool2d and its adjoint
# --------------------------------------------------------------------------- #
P2_MAPS = [(13, 11), (16, 20), (5, 5), (17, 9)]
P2_KSP = [(5, 2, 2), (9, 4, 4), (17, 8, 8), (3, 1, 1), (2, 2, 0), (3, 3, 0), (4, 3, 2)]


def _fits(hw, k, p):
    return hw[0] + 2 * p - k >= 0 and hw[1] + 2 * p - k >= 0


@functools.lru_cache(maxsize=None)
def _pool2_case(hw, c, ksp, dt):
    k, s, p = ksp
    x = q(gen(('p2', hw, c, ksp), 2, c, *hw), dt)
    xr = x.double().requires_grad_(True)
    y = F.avg_pool2d(xr, k, s, p)
    dy = q(gen(('p2dy', hw, c, ksp), *y.shape), dt)
    y.backward(dy.double())
    return x, y.detach(), dy, xr.grad


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('c', [1, 3, 8])
def test_avgpool2d_and_adjoint(be, c, dt):
    from led_net_amd import ops
    uncovered = 0
    for hw in P2_MAPS:
        for ksp in P2_KSP:
            k, s, p = ksp
            if not _fits(hw, k, p):
                continue
            x, y, dy, dx = _pool2_case(hw, c, ksp, dt)
            what = f'{hw} k{k} s{s} p{p} C{c} {DT_IDS[dt]}'
            got = ops.avgpool2d(be(nhwc(x).to(dt)), k, s, p)
            assert got.dtype == dt and tuple(got.shape[1:3]) == tuple(y.shape[2:])
            check(be, f'avgpool2d {DT_IDS[dt]}', nchw(got), y, out_bound(dt, TOL_F32), what)
            gdx = nchw(ops.avgpool2d_bwd(be(nhwc(dy).to(dt)), hw, k, s, p))
            check(be, f'avgpool2d_bwd {DT_IDS[dt]}', gdx, dx, out_bound(dt, TOL_F32), what)
            # rows / columns past the last window receive no gradient: exactly 0
            ye, xe = (y.shape[2] - 1) * s - p + k, (y.shape[3] - 1) * s - p + k
            if ye < hw[0]:
                uncovered += 1
                assert bool((gdx[:, :, ye:, :] == 0).all()), what
            if xe < hw[1]:
                uncovered += 1
                assert bool((gdx[:, :, :, xe:] == 0).all()), what
    assert uncovered > 0          # (3,3,0) and (4,3,2) leave trailing rows on these maps


def test_avgpool2d_rejections(be):
    from led_net_amd import _lib, ops
    x = be(torch.zeros(1, 8, 8, 4))
    with pytest.raises(ops.LednError):
        ops.avgpool2d(x, 3, 1, 2)                   # 2 * pad > k
    with pytest.raises(ops.LednError):
        ops.avgpool2d_bwd(be(torch.zeros(1, 10, 10, 4)), (8, 8), 3, 1, 2)
    # a wrong Ho through the raw library call: k 3, s 2, p 1 on 8 x 8 gives 4 x 4
    lib = _lib.get_lib()
    y = be(torch.zeros(1, 5, 5, 4))
    args = (1, 8, 8, 4)
    assert lib.cdll.ledn_avgpool2d(x.data_ptr(), y.data_ptr(), *args, 4, 4, 3, 2, 1, _lib.F32, raw_stream(x)) == _lib.OK
    assert lib.cdll.ledn_avgpool2d(x.data_ptr(), y.data_ptr(), *args, 5, 4, 3, 2, 1, _lib.F32, raw_stream(x)) == _lib.EINVAL
    assert lib.cdll.ledn_avgpool2d_bwd(y.data_ptr(), x.data_ptr(), *args, 5, 4, 3, 2, 1, _lib.F32, raw_stream(x)) == _lib.EINVAL


# --------------------------------------------------------------------------- #
# 8. GETB mixing pass and its adjoint
# --------------------------------------------------------------------------- #
GP_MAPS = [(2, 2), (3, 5), (4, 9), (8, 8), (13, 11), (7, 2)]     # maps below ws / 2: reflected row H meets the window clipping


@functools.lru_cache(maxsize=None)
def _getb_case(hw, c, ws, dt):
    a = q(gen(('gpa', hw, c, ws), 2, c, *hw), dt)
    local = q(gen(('gpl', hw, c, ws), 2, c, *hw), dt)
    ar = a.double().requires_grad_(True)
    out = F.avg_pool2d(F.pad(ar, (0, 0, 0, 1), mode='reflect'), (ws, 1), 1, (ws // 2 - 1, 0)) + \
        F.avg_pool2d(F.pad(ar, (0, 1, 0, 0), mode='reflect'), (1, ws), 1, (0, ws // 2 - 1)) + local.double()
    dout = q(gen(('gpd', hw, c, ws), 2, c, *hw), dt)
    out.backward(dout.double())
    return a, local, out.detach(), dout, ar.grad


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('c', [4, 12, 32])
@pytest.mark.parametrize('ws', [8, 4, 2])
def test_getb_pool_and_adjoint(be, ws, c, dt):
    from led_net_amd import ops, ops_train as T
    for hw in GP_MAPS:
        a, local, out, dout, da = _getb_case(hw, c, ws, dt)
        what = f'{hw} ws{ws} C{c} {DT_IDS[dt]}'
        got = ops.getb_pool(be(nhwc(a).to(dt)), be(nhwc(local).to(dt)), ws)
        assert got.dtype == dt
        check(be, f'getb_pool {DT_IDS[dt]}', nchw(got), out, out_bound(dt, TOL_F32), what)
        gda = T.getb_pool_bwd(be(nhwc(dout).to(dt)), ws)
        check(be, f'getb_pool_bwd {DT_IDS[dt]}', nchw(gda), da, out_bound(dt, TOL_F32), what)


def test_getb_pool_rejections(be):
    from led_net_amd import ops, ops_train as T
    for shape in [(1, 4, 4, 6), (1, 1, 4, 4)]:          # C % 4 != 0; H = 1 (no row to reflect)
        z = be(torch.zeros(*shape))
        with pytest.raises(ops.LednError):
            ops.getb_pool(z, z.clone(), 8)
        with pytest.raises(ops.LednError):
            T.getb_pool_bwd(z, 8)


# --------------------------------------------------------------------------- #
# 9. relative-position bias and its adjoint
# --------------------------------------------------------------------------- #
def relpos_index(ws):
    """the module's relative_position_index buffer (blocks._GLA)"""
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing='ij')).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def relpos_gather(table, index):
    """biasT[h][j][i] = table[index[i][j]][h], 0 where the index is outside the table"""
    R = table.shape[0]
    ok = (index >= 0) & (index < R)
    g = table[index.clamp(0, R - 1)] * ok.unsqueeze(-1).to(table.dtype)       # [i][j][h]
    return g.permute(2, 1, 0).contiguous()


def relpos_scatter(dbias, index, dtable0):
    """f64 adjoint of relpos_gather accumulated into dtable0"""
    R, heads = dtable0.shape
    out = dtable0.double().clone()
    flat = index.reshape(-1)
    ok = (flat >= 0) & (flat < R)
    for h in range(heads):
        v = dbias[h].double().t().reshape(-1)          # [i][j]
        out[:, h].index_add_(0, flat[ok], v[ok])
    return out


RP_CASES = [(8, 2), (8, 8), (4, 3), (2, 1), (16, 2)]      # ws 16: R = 961, the largest table under the 1024 limit


@pytest.mark.parametrize('ws,heads', RP_CASES)
def test_relpos_bias_forward(be, ws, heads):
    from led_net_amd import ops
    R, T = (2 * ws - 1) ** 2, ws * ws
    index = relpos_index(ws)
    assert tuple(index.shape) == (T, T) and int(index.max()) == R - 1 and int(index.min()) == 0
    table = gen(('rpt', ws, heads), R, heads)
    got = ops.relpos_bias(be(table), be(index))
    assert torch.equal(got.cpu(), relpos_gather(table, index))
    bad = index.clone()
    bad.view(-1)[[0, T + 1, T * T - 1]] = -1
    bad.view(-1)[[1, 2 * T - 1, T * T - 2]] = R
    got = ops.relpos_bias(be(table), be(bad))
    want = relpos_gather(table, bad)
    assert torch.equal(got.cpu(), want) and int((want == 0).sum()) >= 4 * heads


@pytest.mark.parametrize('ws,heads', RP_CASES)
def test_relpos_bias_bwd(be, ws, heads):
    from led_net_amd import ops
    R, T = (2 * ws - 1) ** 2, ws * ws
    index = relpos_index(ws)
    index.view(-1)[[0, T * T - 1]] = torch.tensor([-1, R])            # two entries outside the table: no gradient
    dbias = gen(('rpd', ws, heads), heads, T, T)
    dtable0 = gen(('rp0', ws, heads), R, heads)
    want = relpos_scatter(dbias, index, dtable0)
    got = {}
    for det in (False, True):
        with deterministic(det):
            got[det] = ops.relpos_bias_bwd(be(dbias), be(index), be(dtable0.clone())).cpu()
        check(be, 'relpos_bias_bwd ' + ('det' if det else 'default'), got[det], want, TOL_F32, f'ws{ws} heads{heads}')
    assert rel_err(got[True], got[False]) <= 1e-6


def test_relpos_bias_bwd_rejects_large_table(be):
    from led_net_amd import _lib
    lib = _lib.get_lib()
    heads, T = 1, 4
    dbias, index, dtable = be(torch.zeros(heads, T, T)), be(torch.zeros(T, T, dtype=torch.int64)), be(torch.zeros(1025, heads))
    args = (dbias.data_ptr(), index.data_ptr(), dtable.data_ptr())
    assert lib.cdll.ledn_relpos_bias_bwd(*args, 1024, heads, T, raw_stream(dbias)) == _lib.OK
    assert lib.cdll.ledn_relpos_bias_bwd(*args, 1025, heads, T, raw_stream(dbias)) == _lib.EINVAL


@pytest.mark.parametrize('det', [False, True], ids=['default', 'deterministic'])
@pytest.mark.parametrize('ws,heads', [(8, 2), (4, 3)])
def test_relpos_bias_bwd_propagates_nonfinite(be, ws, heads, det):
    """a NaN / Inf in the bias gradient makes exactly the table entries (index, head) it maps to non-finite, in both
    modes; every other entry stays finite and correct (the fixed-point form used to clamp them into +-8e6)"""
    from led_net_amd import ops
    R, T = (2 * ws - 1) ** 2, ws * ws
    index = relpos_index(ws)
    dbias = gen(('rpnf', ws, heads), heads, T, T)
    dtable0 = gen(('rpnf0', ws, heads), R, heads)
    (h0, i0, j0), (h1, i1, j1) = (0, 3, T - 2), (heads - 1, T - 1, 1)
    clean = dbias.clone()
    clean[h0, j0, i0] = clean[h1, j1, i1] = 0.0
    dbias[h0, j0, i0], dbias[h1, j1, i1] = float('nan'), float('inf')          # layout [h][key j][query i]
    r0, r1 = int(index[i0, j0]), int(index[i1, j1])
    assert (r0, h0) != (r1, h1)
    want = relpos_scatter(clean, index, dtable0)
    with deterministic(det):
        got = ops.relpos_bias_bwd(be(dbias), be(index), be(dtable0.clone())).cpu()
    assert not bool(torch.isfinite(got[r0, h0])) and not bool(torch.isfinite(got[r1, h1])), (got[r0, h0], got[r1, h1])
    assert bool(torch.isnan(got[r0, h0])) and float(got[r1, h1]) == float('inf')
    mask = torch.ones(R, heads, dtype=torch.bool)
    mask[r0, h0] = mask[r1, h1] = False
    assert bool(torch.isfinite(got[mask]).all())
    check(be, 'relpos_bias_bwd ' + ('det' if det else 'default'), got[mask], want[mask], TOL_F32, f'ws{ws} heads{heads} nonfinite')
