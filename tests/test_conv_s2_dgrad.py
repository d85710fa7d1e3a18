"""Data gradient of the 3x3 stride-2 convolutions as four parity sub-convolutions (conv_s2dgrad_mfma_kernel,
LEDN_OPT_S2_DGRAD = 1) against torch autograd on bf16-rounded operands and against the zero-upsampled form
(LEDN_OPT_S2_DGRAD = 0) on the same operands.  Runs on the emulator and on the GPU."""
import pytest
import torch
import torch.nn.functional as F

OPT_CONV_WORKGROUPS = 0
OPT_DETERMINISTIC = 3
OPT_S2_DGRAD = 6

# (Cin_f, Cout_f, forward input H x W, LEDN_OPT_CONV_WORKGROUPS or 0)
CASES = [
    (32, 32, (16, 64), 0),     # exactly one MT = 2 tile
    (32, 32, (21, 70), 0),     # odd H, ragged W
    (32, 32, (22, 67), 0),     # even H, odd W: the last output row and column read the zero halo
    (64, 128, (18, 40), 0),    # four K-chunks, two dx channel slices
    (128, 256, (10, 36), 0),   # eight K-chunks
    (16, 32, (9, 34), 0),      # dx channel tail of 16
    (32, 48, (9, 34), 0),      # dz channel tail of 16
    (32, 32, (1, 2), 0),       # maps smaller than a tile, Ho = 1
    (32, 32, (2, 1), 0),
    (32, 32, (3, 3), 0),
    (32, 64, (40, 67), 3),     # three workgroups: each walks several tiles and chunks through the pipelined loop
]


def r16(t):
    return t.bfloat16().float()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu().float()


class Case:
    """operands, the torch reference and the four library results of one case, computed once"""

    def __init__(self, be, cin, cout, hw, wgs):
        from led_net_amd import _lib, ops
        lib = _lib.get_lib()
        g = torch.Generator().manual_seed(cin * 1000 + cout + hw[0] * 7 + hw[1])
        x = r16(torch.randn(2, cin, *hw, generator=g)).requires_grad_(True)
        w = r16(torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5)
        z = F.conv2d(x, w, stride=2, padding=1)
        dz = r16(torch.randn(z.shape, generator=g))
        z.backward(dz)
        self.ref = x.grad.detach()
        self.addend = r16(torch.randn(2, cin, *hw, generator=g))

        def dev(t):
            return t.detach().permute(0, 2, 3, 1).contiguous().to(be.dev).bfloat16()
        dzd, wd, addd = dev(dz), w.to(be.dev), dev(self.addend)
        wp = ops.pack_conv_weights(wd, 1)
        kw = dict(stride=2, pad=1, out_hw=hw, w_bf16=wp)
        kwa = dict(kw, res=addd, res_mode=ops.RES_ADD)
        self.run = lambda add: ops.conv2d(dzd, wd, transposed=True, **(kwa if add else kw))
        if wgs:
            lib.set_option(OPT_CONV_WORKGROUPS, wgs)
        try:
            self.applies = (ops.conv2d_s2_dgrad_applies(dzd, wd, **kw), ops.conv2d_s2_dgrad_applies(dzd, wd, **kwa))
            self.new = (nchw(self.run(False)), nchw(self.run(True)))
            lib.set_option(OPT_S2_DGRAD, 0)
            self.applies_off = ops.conv2d_s2_dgrad_applies(dzd, wd, **kw)
            self.old = (nchw(self.run(False)), nchw(self.run(True)))
        finally:
            lib.set_option(OPT_S2_DGRAD, 1)
            if wgs:
                lib.set_option(OPT_CONV_WORKGROUPS, 0)


_CACHE = {}


@pytest.fixture(params=CASES, ids=lambda c: f'{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}' + (f'-wg{c[3]}' if c[3] else ''))
def case(be, request):
    key = (str(be.dev), request.param)
    if key not in _CACHE:
        _CACHE[key] = Case(be, *request.param)
    c = _CACHE[key]
    # no case passes on the fallback
    assert c.applies == (True, True) and c.applies_off is False
    return c


def test_s2_dgrad_against_torch(case):
    """the bounds of test_conv_mfma.py::test_mfma_conv_dgrad_wgrad (no addend) and
    ::test_mfma_dgrad_accumulates_partial_gradient (bf16 addend)"""
    torch.testing.assert_close(case.new[0], case.ref, rtol=2e-2, atol=2e-2 * float(case.ref.abs().max()))
    torch.testing.assert_close(case.new[1], case.ref + case.addend, rtol=2e-2, atol=3e-2)


def test_s2_dgrad_against_zero_upsampled_form(case):
    """both forms accumulate in f32 and round once to bf16: at most one bf16 ulp apart, except where the f32
    reordering noise exceeds an ulp of a nearly cancelled result"""
    for new, old in zip(case.new, case.old):
        print('max |new - old| = %.3e, max |old| = %.3e' % (float((new - old).abs().max()), float(old.abs().max())))
        torch.testing.assert_close(new, old, rtol=2.0 ** -7, atol=1e-3 * float(old.abs().max()))


@pytest.mark.parametrize('det', [0, 1])
def test_s2_dgrad_repeatable(be, case, det):
    """every output element is written once, by one lane: two calls give identical bits in default and in
    deterministic mode"""
    from led_net_amd import _lib
    lib = _lib.get_lib()
    lib.set_option(OPT_DETERMINISTIC, det)
    try:
        for add in (False, True):
            a, b = case.run(add), case.run(add)
            assert torch.equal(a, b)
            assert torch.equal(nchw(a), case.new[int(add)])     # (and the mode changes nothing)
    finally:
        lib.set_option(OPT_DETERMINISTIC, 0)
