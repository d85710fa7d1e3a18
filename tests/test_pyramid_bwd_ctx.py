"""Context-branch SESP pyramid data gradient straight from dy (csrc/stencil_bf16.hip pyr_bwd_data_ctx_kernel: unequal
dilations, stride 1 and 2, dy patch staged once in LDS, no suffix-sum pass) and the 16-byte-per-lane adjoint of the 3x3/s2
average pool (csrc/backward.hip avgpool3x3s2_bwd_quad_kernel), against torch autograd in f32 on the same bf16-rounded
operands and against the generic kernels behind the same C-ABI entries (LEDN_OPT_STREAM_FAST = 0).  N = 2 so that a halo
that read the neighbouring image would show.  Emulator on CPU; the same tests on the MI355X with -m gpu."""
import pytest
import torch
import torch.nn.functional as F

torch.manual_seed(11)
BF = torch.bfloat16
OPT_STREAM_FAST = 2


def r16(t):
    return t.to(BF).float()


def nhwc16(be, t):
    return be(t.detach().permute(0, 2, 3, 1).contiguous().to(BF))


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu().float()


def close16(got, want, tol):
    """bf16 output rounding: relative to the tensor's scale"""
    scale = float(want.abs().max()) + 1e-6
    err = float((got - want).abs().max())
    assert err <= tol * scale, (err, scale)


def _fast(on):
    from led_net_amd import _lib
    _lib.get_lib().set_option(OPT_STREAM_FAST, -1 if on else 0)      # -1: the default mask


def _pyramid_case(n, hw, stride, dil):
    """operands and the autograd reference of test_stencil_bf16.test_sesp_pyramid_bf16_fwd_bwd"""
    x = r16(torch.randn(2, n, *hw)).requires_grad_(True)
    ws = [(torch.randn(n, 1, 3, 3) * 0.3).requires_grad_(True) for _ in range(4)]
    outs = []
    for i in range(4):
        o = F.conv2d(x, ws[i], stride=stride, padding=dil[i], dilation=dil[i], groups=n)
        outs.append(o if i == 0 else o + outs[-1])
    y = torch.cat(outs, 1)
    wp = torch.stack([w[:, 0].permute(1, 2, 0) for w in ws]).detach().contiguous()
    dy = r16(torch.randn_like(y))
    y.backward(dy)
    want_dw = torch.stack([w.grad[:, 0].permute(1, 2, 0) for w in ws])
    return x, dy, wp, x.grad, want_dw


ASC = (1, 2, 3, 4)
PYR_CASES = [
    # stride 1: ragged in both directions; map smaller than the tile with fewer rows than twice the halo; several tiles
    (1, ASC, 8, (13, 21)), (1, ASC, 16, (9, 40)), (1, ASC, 128, (5, 6)), (1, ASC, 32, (33, 70)),
    # stride 2: odd H; odd W; smaller than the halo; several tiles of even size
    (2, ASC, 16, (13, 10)), (2, ASC, 32, (8, 9)), (2, ASC, 64, (3, 5)), (2, ASC, 8, (34, 66)),
    # non-ascending and equal dilations
    (1, (3, 1, 4, 2), 16, (11, 19)), (2, (3, 1, 4, 2), 16, (11, 19)),
    (1, (2, 2, 2, 2), 16, (11, 19)), (2, (2, 2, 2, 2), 16, (11, 19)),
]


@pytest.mark.parametrize('stride,dil,n,hw', PYR_CASES)
def test_pyramid_bwd_ctx(be, stride, dil, n, hw):
    """dx within 3e-2 of the tensor's scale and dw at rtol 2e-2 / atol 2e-2 max|dw| of autograd (the suffix sums are
    rounded to bf16 before the gather, as in gsum); dx of the tiled kernel within the same bound of the generic path's --
    and equal to it, since the patch holds what gsum held and the taps are added in the generic kernels' order."""
    from led_net_amd import ops_train as T
    dil = list(dil)
    x, dy, wp, want_dx, want_dw = _pyramid_case(n, hw, stride, dil)
    xd, dyd, wd = nhwc16(be, x), nhwc16(be, dy), be(wp)
    try:
        _fast(True)
        # every one of these shapes is inside the new kernel's gate (bf16, n = 8 * 2^k, halos <= 4): it must serve them
        assert T.PYR_BWD_KERNELS[T.sesp_pyramid_bwd_kernel_id(xd, dyd, dil, stride)] == 'pyr_bwd_data_ctx_kernel'
        dx, dw = T.sesp_pyramid_bwd(xd, dyd, wd, dil, stride)
        _fast(False)
        assert T.sesp_pyramid_bwd_kernel_id(xd, dyd, dil, stride) == (1 if stride == 1 else 0)
        dx0, dw0 = T.sesp_pyramid_bwd(xd, dyd, wd, dil, stride)
    finally:
        _fast(True)
    close16(nchw(dx), want_dx, 3e-2)
    torch.testing.assert_close(dw.cpu(), want_dw, rtol=2e-2, atol=2e-2 * float(want_dw.abs().max()))
    close16(nchw(dx0), want_dx, 3e-2)
    close16(nchw(dx), nchw(dx0), 3e-2)
    print(f'max|dx - dx_generic| = {float((dx.float() - dx0.float()).abs().max()):.3e}')
    assert torch.equal(dx, dx0)
    torch.testing.assert_close(dw0.cpu(), want_dw, rtol=2e-2, atol=2e-2 * float(want_dw.abs().max()))


def test_pyramid_bwd_ctx_f32_keeps_generic_path(be):
    from led_net_amd import ops_train as T
    x, dy = be(torch.randn(2, 9, 12, 16)), be(torch.randn(2, 9, 12, 64))
    assert T.sesp_pyramid_bwd_kernel_id(x, dy, [1, 2, 3, 4], 1) == 0                      # f32
    xb, dyb = be(torch.randn(2, 9, 12, 12).to(BF)), be(torch.randn(2, 9, 12, 48).to(BF))
    assert T.sesp_pyramid_bwd_kernel_id(xb, dyb, [1, 2, 3, 4], 1) == 0                    # n % 8 != 0
    x16, dy16 = be(torch.randn(2, 9, 12, 16).to(BF)), be(torch.randn(2, 9, 12, 64).to(BF))
    assert T.sesp_pyramid_bwd_kernel_id(x16, dy16, [1, 2, 3, 9], 1) == 1                  # halo beyond the LDS image
    assert T.sesp_pyramid_bwd_kernel_id(x16, dy16, [4, 4, 4, 4], 1) == 1                  # patches beyond the LDS image


@pytest.mark.parametrize('stride,n,hw', [(1, 32, (33, 70)), (2, 16, (13, 10))])
def test_pyramid_bwd_ctx_deterministic(be, stride, n, hw):
    """deterministic mode: two calls on the same inputs are bit-identical for dx (a gather) and for dw"""
    import led_net_amd as L
    from led_net_amd import ops_train as T
    x, dy, wp, _, _ = _pyramid_case(n, hw, stride, list(ASC))
    xd, dyd, wd = nhwc16(be, x), nhwc16(be, dy), be(wp)
    L.set_deterministic(True)
    try:
        _fast(True)
        a = T.sesp_pyramid_bwd(xd, dyd, wd, list(ASC), stride)
        b = T.sesp_pyramid_bwd(xd, dyd, wd, list(ASC), stride)
    finally:
        L.set_deterministic(False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('shape', [(2, 13, 10, 16), (1, 8, 9, 64), (2, 3, 5, 8), (1, 34, 66, 128)])
@pytest.mark.parametrize('with_add', [False, True])
def test_avgpool_bwd_quad(be, shape, with_add):
    """bit-identical to the generic kernel; against autograd of F.avg_pool2d(x, 3, 2, 1) at test_ops_bwd's tolerance
    (rtol 2e-4, atol 2e-5) for the f32 result, to which the bf16 output adds its own rounding: half a bf16 ulp,
    2^-8 |want| (8 significand bits) -- a bound no bf16 tensor can do without."""
    from led_net_amd import ops_train as T
    N, H, W, C = shape
    x = torch.zeros(N, C, H, W, requires_grad=True)
    y = F.avg_pool2d(x, 3, 2, 1)
    dy = r16(torch.randn_like(y))
    y.backward(dy)
    add = r16(torch.randn(N, C, H, W)) if with_add else None
    want = x.grad + add if with_add else x.grad
    dyd, addd = nhwc16(be, dy), nhwc16(be, add) if with_add else None
    try:
        _fast(True)
        got = T.avgpool3x3s2_bwd(dyd, (H, W), add=addd)
        _fast(False)
        gen = T.avgpool3x3s2_bwd(dyd, (H, W), add=addd)
    finally:
        _fast(True)
    assert got.dtype == BF and torch.equal(got, gen)
    err = (nchw(got) - want).abs()
    bound = 2e-5 + (2e-4 + 2.0 ** -8) * want.abs()
    print(f'max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all())
