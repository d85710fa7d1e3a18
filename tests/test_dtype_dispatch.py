"""Every entry of the C ABI answers a dtype code, or a combination of codes, that it has no kernel for with LEDN_EINVAL
and launches nothing (csrc/ledn_rt.h: with_dtype).  Each case first runs the entry with float32 everywhere -- the shape
is one its validator accepts, so the rejection that follows is the dtype's -- then refills the outputs with a sentinel,
repeats the call with the unsupported code and expects LEDN_EINVAL and bit-unchanged outputs.  All buffers are float32
sized, so a kernel wrongly launched for a narrower type would stay in bounds and show up as an assertion."""
import ctypes as C

import pytest
import torch

import led_net_amd  # noqa: F401
from led_net_amd import _lib as L

SENTINEL = -1234.5
BAD = 7                 # not a LEDN_* dtype code


class Ctx:
    def __init__(self, be):
        self.be = be
        self.lib = L.get_lib()
        self.stream = torch.cuda.current_stream(be.dev).cuda_stream if self.lib.is_hip else None

    def buf(self, n, fill=None):
        t = torch.full((n,), SENTINEL) if fill is None else torch.full((n,), float(fill))
        return self.be(t)

    def ints(self, n):
        return self.be(torch.zeros(n, dtype=torch.int32))

    def call(self, name, *args):
        rc = getattr(self.lib.cdll, name)(*args)
        if self.lib.is_hip:
            torch.cuda.synchronize()
        return rc


def untouched(t):
    return bool((t.cpu().view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32)).all())


def expect_rejected(cx, outs, run, good, bad_sets):
    """run(dtypes) -> return code; good: the all-float32 dtype tuple; bad_sets: the tuples that must be refused"""
    assert run(good) == L.OK, 'the float32 call must be accepted: the shape of this case is wrong'
    for bad in bad_sets:
        for o in outs:
            o.fill_(SENTINEL)
        assert run(bad) == L.EINVAL, f'dtypes {bad} were not refused'
        for i, o in enumerate(outs):
            assert untouched(o), f'dtypes {bad}: output {i} was written'


def resize_desc(x, y, nchw, dx, dy):
    return L.ResizeDesc(x=x.data_ptr(), add=None, y=y.data_ptr(), argmax=None, N=1, H=4, W=4, C=2, Ho=8, Wo=8,
                        out_nchw=nchw, dtype_x=dx, dtype_y=dy)


@pytest.mark.parametrize('dtype_x', [L.U8, BAD])
def test_bilinear_nchw_refuses_unsupported_input(be, dtype_x):
    """the planar-output ladder used to end in `else <bf16 kernel>`: ledn_bilinear(out_nchw=1) with an 8-bit or unknown
    dtype_x launched bilinear_nchw_kernel<bf16_t, C> on the caller's buffer and returned LEDN_OK"""
    cx = Ctx(be)
    x, y = cx.buf(1 * 4 * 4 * 2, fill=1.0), cx.buf(1 * 2 * 8 * 8)
    rc = cx.call('ledn_bilinear', C.byref(resize_desc(x, y, 1, dtype_x, L.F32)), cx.stream)
    assert rc == L.EINVAL
    assert untouched(y)


def test_bilinear_nhwc(be):
    cx = Ctx(be)
    x, y = cx.buf(1 * 4 * 4 * 2, fill=1.0), cx.buf(1 * 8 * 8 * 2)
    expect_rejected(cx, [y], lambda dt: cx.call('ledn_bilinear', C.byref(resize_desc(x, y, 0, *dt)), cx.stream),
                    (L.F32, L.F32), [(BAD, L.F32), (L.F32, BAD), (L.U8, L.F32)])


def test_bilinear_nchw_output_dtype(be):
    cx = Ctx(be)
    x, y = cx.buf(1 * 4 * 4 * 2, fill=1.0), cx.buf(1 * 2 * 8 * 8)
    expect_rejected(cx, [y], lambda dt: cx.call('ledn_bilinear', C.byref(resize_desc(x, y, 1, *dt)), cx.stream),
                    (L.F32, L.F32), [(L.F32, L.BF16), (L.F32, BAD)])


def test_affine_act(be):
    cx = Ctx(be)
    x, y = cx.buf(2 * 4, fill=1.0), cx.buf(2 * 4)

    def run(dt):
        d = L.AffineDesc(x=x.data_ptr(), y=y.data_ptr(), P=2, C=4, act=L.ACT_RELU, res_mode=L.RES_NONE,
                         dtype_x=dt[0], dtype_y=dt[1])
        return cx.call('ledn_affine_act', C.byref(d), cx.stream)
    expect_rejected(cx, [y], run, (L.F32, L.F32), [(BAD, L.F32), (L.F32, BAD), (L.U8, L.F32)])


@pytest.mark.parametrize('entry', ['ledn_bn_act_bwd_reduce', 'ledn_bn_act_bwd_apply'])
def test_bn_act_bwd(be, entry):
    cx = Ctx(be)
    z, dy = cx.buf(2 * 4, fill=1.0), cx.buf(2 * 4, fill=1.0)
    sum_g, sum_gx, dz = cx.buf(4), cx.buf(4), cx.buf(2 * 4)

    def run(dt):
        d = L.BnBwdDesc(z=z.data_ptr(), dy=dy.data_ptr(), sum_g=sum_g.data_ptr(), sum_gx=sum_gx.data_ptr(),
                        dz=dz.data_ptr(), count=2.0, P=2, C=4, act=L.ACT_RELU, res_mode=L.RES_NONE, bn_mode=0,
                        dtype_z=dt[0], dtype_y=dt[1])
        return cx.call(entry, C.byref(d), cx.stream)
    expect_rejected(cx, [sum_g, sum_gx, dz], run, (L.F32, L.F32), [(BAD, L.F32), (L.F32, BAD)])


def test_dwconv2d(be):
    cx = Ctx(be)
    x, w, y = cx.buf(2 * 2 * 4, fill=1.0), cx.buf(9 * 4, fill=1.0), cx.buf(2 * 2 * 4)

    def run(dt):
        d = L.DwDesc(x=x.data_ptr(), w=w.data_ptr(), y=y.data_ptr(), N=1, H=2, W=2, C=4, Ho=2, Wo=2, KH=3, KW=3,
                     stride=1, pad=1, dil=(C.c_int * 4)(1, 1, 1, 1), group_size=4, act_out=L.ACT_NONE, ext1=0,
                     dtype_x=dt[0], dtype_y=dt[1])
        return cx.call('ledn_dwconv2d', C.byref(d), cx.stream)
    expect_rejected(cx, [y], run, (L.F32, L.F32), [(BAD, L.F32), (L.F32, BAD)])


@pytest.mark.parametrize('entry', ['ledn_dwconv2d_bwd_data', 'ledn_dwconv2d_bwd_weight', 'ledn_dwconv2d_bwd'])
def test_dwconv2d_bwd(be, entry):
    cx = Ctx(be)
    x, dz, w = cx.buf(2 * 2 * 4, fill=1.0), cx.buf(2 * 2 * 4, fill=1.0), cx.buf(9 * 4, fill=1.0)
    dx, dw = cx.buf(2 * 2 * 4), cx.buf(9 * 4)

    def run(dt):
        d = L.DwBwdDesc(x=x.data_ptr(), dz=dz.data_ptr(), w=w.data_ptr(), dx=dx.data_ptr(), dw=dw.data_ptr(), N=1, H=2,
                        W=2, C=4, Ho=2, Wo=2, KH=3, KW=3, stride=1, pad=1, dil=(C.c_int * 4)(1, 1, 1, 1), group_size=4,
                        ext1=0, dtype=dt[0])
        return cx.call(entry, C.byref(d), cx.stream)
    expect_rejected(cx, [dx, dw], run, (L.F32,), [(BAD,), (L.U8,)])


def test_sesp_pyramid(be):
    """the pyramid forward has no mixed-dtype kernels: (f32, bf16) is a combination to refuse, not only an unknown code"""
    cx = Ctx(be)
    x, w, y = cx.buf(2 * 2 * 4, fill=1.0), cx.buf(4 * 9 * 4, fill=1.0), cx.buf(2 * 2 * 16)

    def run(dt):
        d = L.PyrDesc(x=x.data_ptr(), w=w.data_ptr(), y=y.data_ptr(), N=1, H=2, W=2, n=4, Ho=2, Wo=2, stride=1,
                      dil=(C.c_int * 4)(1, 2, 3, 4), dtype_x=dt[0], dtype_y=dt[1])
        return cx.call('ledn_sesp_pyramid', C.byref(d), cx.stream)
    expect_rejected(cx, [y], run, (L.F32, L.F32), [(BAD, BAD), (L.F32, L.BF16), (L.BF16, L.F32)])


@pytest.mark.parametrize('entry', ['ledn_sesp_pyramid_bwd_data', 'ledn_sesp_pyramid_bwd_weight'])
def test_sesp_pyramid_bwd(be, entry):
    cx = Ctx(be)
    x, dy, w = cx.buf(2 * 2 * 4, fill=1.0), cx.buf(2 * 2 * 16, fill=1.0), cx.buf(4 * 9 * 4, fill=1.0)
    gsum, dx, dw = cx.buf(2 * 2 * 16), cx.buf(2 * 2 * 4), cx.buf(4 * 9 * 4)

    def run(dt):
        d = L.PyrBwdDesc(x=x.data_ptr(), dy=dy.data_ptr(), w=w.data_ptr(), gsum=gsum.data_ptr(), dx=dx.data_ptr(),
                         dw=dw.data_ptr(), N=1, H=2, W=2, n=4, Ho=2, Wo=2, stride=1, dil=(C.c_int * 4)(1, 2, 3, 4),
                         dtype=dt[0])
        return cx.call(entry, C.byref(d), cx.stream)
    expect_rejected(cx, [gsum, dx, dw], run, (L.F32,), [(BAD,), (L.U8,)])


def test_nchw_to_nhwc(be):
    """five of the nine combinations have a kernel; bf16 -> f32 is a valid pair of codes without one"""
    cx = Ctx(be)
    x, y = cx.buf(1 * 3 * 2 * 2, fill=1.0), cx.buf(1 * 2 * 2 * 3)

    def run(dt):
        return cx.call('ledn_nchw_to_nhwc', x.data_ptr(), dt[0], y.data_ptr(), dt[1], 1, 3, 2, 2, None, None, None, None,
                       C.c_float(0.0), cx.stream)
    expect_rejected(cx, [y], run, (L.F32, L.F32), [(BAD, L.F32), (L.F32, BAD), (L.BF16, L.F32), (L.F32, L.U8)])
