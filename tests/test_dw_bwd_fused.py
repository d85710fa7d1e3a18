"""Fused depthwise 3x3 backward (csrc/dwconv.hip dw3x3_bwd_tile_kernel behind ledn_dwconv2d_bwd): dx and dw from one
staging of dz.  Every case first asserts that ledn_dwconv2d_bwd_fused_applies says yes, so none passes on the fallback.
  dx: bit-identical to ledn_dwconv2d_bwd_data (same FMAs in the same order).
  dw: the unfused kernel's sum in another order of f32 additions: against torch autograd in f32 on the same bf16-rounded
      operands AND against ledn_dwconv2d_bwd_weight it keeps the bound tests/test_stencil_bf16.py sets for this gradient,
      rtol 2e-3, atol 2e-3 * max|dw|.
  Two calls on the same inputs give the same bits, in default and in deterministic mode (no float atomic meets another).
Shapes are N,H,W,C with group size C/4, the smallest that pass the gate of 16384 pixels; N = 2 where a halo read into the
neighbouring image must show.  Emulator on the CPU; the same cases on the MI355X with -m gpu."""
import pytest
import torch
import torch.nn.functional as F

BF = torch.bfloat16
OPT_DW_BWD_WORKGROUPS = 5

CASES = [
    ((2, 96, 96, 32), (2, 2, 2, 2)),        # exact tiles, group size 8
    ((2, 90, 100, 64), (2, 2, 2, 2)),       # ragged in both directions
    ((1, 70, 250, 64), (2, 3, 4, 5)),       # HL = 5 instance; a 32-channel slice spanning two dilations
    ((2, 33, 260, 128), (2, 3, 4, 5)),      # one dilation per slice
    ((1, 8, 2048, 32), (1, 1, 1, 1)),       # map lower than one tile
]
_REF = {}


def r16(t):
    return t.to(BF).float()


def _case(shape, dil):
    """operands (NCHW f32, bf16-rounded) and the autograd reference, computed once per shape and left unchanged"""
    key = (shape, dil)
    if key not in _REF:
        N, H, W, C = shape
        n = C // 4
        g = torch.Generator().manual_seed(17 + H + C)
        x = r16(torch.randn(N, C, H, W, generator=g)).requires_grad_(True)
        ws = [(torch.randn(n, 1, 3, 3, generator=g) * 0.3).requires_grad_(True) for _ in range(4)]
        z = torch.cat([F.conv2d(x[:, i * n:(i + 1) * n], ws[i], padding=dil[i], dilation=dil[i], groups=n)
                       for i in range(4)], 1)
        dz = r16(torch.randn(N, C, H, W, generator=g))
        add = r16(torch.randn(N, C, H, W, generator=g))
        z.backward(dz)
        wp = torch.cat([w[:, 0].permute(1, 2, 0) for w in ws], 2).detach().contiguous()
        want_dw = torch.cat([w.grad[:, 0].permute(1, 2, 0) for w in ws], 2)
        _REF[key] = (x.detach(), dz, add, wp, x.grad, want_dw)
    return _REF[key]


def nhwc16(be, t):
    return be(t.permute(0, 2, 3, 1).contiguous().to(BF))


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu().float()


def _operands(be, shape, dil, with_add):
    x, dz, add, wp, want_dx, want_dw = _case(shape, dil)
    kw = dict(dil=list(dil), group_size=shape[3] // 4)
    return nhwc16(be, x), nhwc16(be, dz), be(wp), (nhwc16(be, add) if with_add else None), kw, \
        (want_dx + add if with_add else want_dx), want_dw


def _dw_close(got, want):
    torch.testing.assert_close(got.cpu(), want.cpu(), rtol=2e-3, atol=2e-3 * float(want.abs().max()))


@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('shape,dil', CASES)
def test_dw_bwd_fused(be, shape, dil, with_add):
    import led_net_amd as L
    from led_net_amd import ops_train as T
    xd, dzd, wd, addd, kw, want_dx, want_dw = _operands(be, shape, dil, with_add)
    assert T.dwconv2d_bwd_fused_applies(xd, dzd, wd, **kw)
    dx, dw = T.dwconv2d_bwd(xd, dzd, wd, add=addd, **kw)
    dx2, dw2 = T.dwconv2d_bwd(xd, dzd, wd, add=addd, **kw)
    # the two entries the fused one replaces
    dx0, _ = T.dwconv2d_bwd(xd, dzd, wd, add=addd, need_dw=False, **kw)
    _, dw0 = T.dwconv2d_bwd(xd, dzd, wd, need_dx=False, **kw)
    assert dx.dtype == BF and torch.equal(dx, dx0) and torch.equal(dx2, dx0)
    scale = float(want_dx.abs().max())
    assert float((nchw(dx) - want_dx).abs().max()) <= 1.5e-2 * scale       # test_stencil_bf16.close16: bf16 output rounding
    print(f'max|dw - autograd| / max|dw| = {float((dw.cpu() - want_dw).abs().max() / want_dw.abs().max()):.3e}, '
          f'max|dw - unfused| / max|dw| = {float((dw - dw0).abs().max() / dw0.abs().max()):.3e}')
    _dw_close(dw, want_dw)
    _dw_close(dw, dw0)
    assert torch.equal(dw, dw2)
    # accumulate-into semantics of the gradient sinks: the one adder of an element adds its sum to what is there
    pre = be(torch.linspace(-3.0, 5.0, dw.numel()).reshape(dw.shape).contiguous())
    sink = pre.clone()
    dx3, dw3 = T.dwconv2d_bwd(xd, dzd, wd, add=addd, dw_out=sink, **kw)
    assert dw3 is sink and torch.equal(dx3, dx0)
    _dw_close(sink - pre, want_dw)
    assert torch.equal(sink, pre + dw)
    L.set_deterministic(True)
    try:
        dxa, dwa = T.dwconv2d_bwd(xd, dzd, wd, add=addd, **kw)
        dxb, dwb = T.dwconv2d_bwd(xd, dzd, wd, add=addd, **kw)
    finally:
        L.set_deterministic(False)
    assert torch.equal(dxa, dx0) and torch.equal(dxb, dx0) and torch.equal(dwa, dwb)
    _dw_close(dwa, want_dw)
    _dw_close(dwa, dw0)


@pytest.mark.parametrize('wgs', [4, 400])
def test_dw_bwd_fused_workgroups(be, wgs):
    """LEDN_OPT_DW_BWD_WORKGROUPS = 4: two workgroups per 32-channel slice walk 24 tiles each; 400: 200 rows per slice for
    48 tiles, so most workgroups get no tile and leave a row of zeros"""
    from led_net_amd import _lib, ops_train as T
    shape, dil = CASES[1]
    xd, dzd, wd, addd, kw, want_dx, want_dw = _operands(be, shape, dil, True)
    assert T.dwconv2d_bwd_fused_applies(xd, dzd, wd, **kw)
    dx0, _ = T.dwconv2d_bwd(xd, dzd, wd, add=addd, need_dw=False, **kw)
    _, dw0 = T.dwconv2d_bwd(xd, dzd, wd, need_dx=False, **kw)
    lib = _lib.get_lib()
    lib.set_option(OPT_DW_BWD_WORKGROUPS, wgs)
    try:
        dx, dw = T.dwconv2d_bwd(xd, dzd, wd, add=addd, **kw)
        dx2, dw2 = T.dwconv2d_bwd(xd, dzd, wd, add=addd, **kw)
    finally:
        lib.set_option(OPT_DW_BWD_WORKGROUPS, 0)      # <= 0: the default
    assert torch.equal(dx, dx0) and torch.equal(dx2, dx0) and torch.equal(dw, dw2)
    _dw_close(dw, want_dw)
    _dw_close(dw, dw0)


def test_dw_bwd_fused_dwfn_sink(be):
    """train.DwFn under autograd with a bank-gradient sink (the default step's form): dx and the sink against the two-call
    path on the same operands"""
    from led_net_amd import ops_train as T, train
    shape, dil = CASES[1]
    xd, dzd, wd, _, kw, _, want_dw = _operands(be, shape, dil, False)
    assert T.dwconv2d_bwd_fused_applies(xd, dzd, wd, **kw)
    dx0, _ = T.dwconv2d_bwd(xd, dzd, wd, need_dw=False, **kw)
    _, dw0 = T.dwconv2d_bwd(xd, dzd, wd, need_dx=False, **kw)
    pre = be(torch.full(tuple(wd.shape), 0.25))
    sink = pre.clone()
    banks = train._DwBanks
    saved = (banks.frozen, dict(banks.by_ptr), banks.pending)
    try:
        banks.frozen, banks.by_ptr = True, {wd.data_ptr(): sink}
        xg = xd.clone().requires_grad_(True)
        z = train.DwFn.apply(xg, wd, 1, -1, tuple(dil), kw['group_size'], False, None)
        z.backward(dzd)
    finally:
        banks.frozen, banks.by_ptr, banks.pending = saved
    assert torch.equal(xg.grad, dx0)
    _dw_close(sink - pre, dw0)
    _dw_close(sink - pre, want_dw)


def _pair_equals_fused_entry(be, x, dz, wd, **kw):
    from led_net_amd import ops_train as T
    assert not T.dwconv2d_bwd_fused_applies(x, dz, wd, **kw)
    dx, dw = T.dwconv2d_bwd(x, dz, wd, **kw)                      # ledn_dwconv2d_bwd: falls back to the pair
    dx0, _ = T.dwconv2d_bwd(x, dz, wd, need_dw=False, **kw)
    _, dw0 = T.dwconv2d_bwd(x, dz, wd, need_dx=False, **kw)
    assert torch.equal(dx, dx0) and torch.equal(dw, dw0)


@pytest.mark.parametrize('be', ['emu'], indirect=True)
def test_dw_bwd_outside_gate_keeps_pair(be):
    """CPU only (the emulator adds in one fixed order, so the fallback's dw is bit-identical to the pair's): descriptors
    outside the gate -- f32, stride 2, C = 48, 4096 pixels -- are refused by ledn_dwconv2d_bwd_fused_applies and get the
    old pair's results through ledn_dwconv2d_bwd"""
    g = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g)
    w64, w48 = be(rn(3, 3, 64) * 0.3), be(rn(3, 3, 48) * 0.3)
    dil = dict(dil=[2, 2, 2, 2])
    _pair_equals_fused_entry(be, be(rn(1, 128, 128, 64)), be(rn(1, 128, 128, 64)), w64, group_size=16, **dil)      # f32
    x = be(rn(1, 128, 128, 64).to(BF))
    _pair_equals_fused_entry(be, x, be(rn(1, 64, 64, 64).to(BF)), w64, stride=2, pad=2, group_size=16, **dil)      # stride 2
    x48 = be(rn(1, 128, 128, 48).to(BF))
    _pair_equals_fused_entry(be, x48, be(rn(1, 128, 128, 48).to(BF)), w48, group_size=24, **dil)                   # C = 48
    xs = be(rn(1, 64, 64, 64).to(BF))
    _pair_equals_fused_entry(be, xs, be(rn(1, 64, 64, 64).to(BF)), w64, group_size=16, **dil)                      # 4096 pixels
