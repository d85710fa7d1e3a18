"""Depthwise 3x3 / 8x8 convolutions, the SESP pyramid and the filter-bank repack, one case per kernel instance the
launchers of csrc/dwconv.hip, csrc/stencil_bf16.hip and the depthwise / pyramid sections of csrc/backward.hip can pick,
against plain torch in float64 on the CPU.  Every case first asserts the kernel id (and, for reductions, the ending) it
was written for through the no-launch ledn_*_kernel_id queries, so none passes on a fallback.

Two kinds of case per instance:

EXACT (`exact=True`): operands are small integers, so every product and partial sum is an integer below 2^24 (exact in
f32 in any order, with atomics or partial rows, on the emulator and on the device) and every output is an integer of at
most 8 significant bits (exact in bf16).  The assertion is torch.equal against the f64 reference cast to the output
type; a failure names the first differing element as (n, y, x, c).  Magnitudes (the reference is checked against them
before it is used):
  3x3            per-channel taps = a seeded permutation of {-4..-1, 1..5}, x / dz in {-2..2}:  |sum| <= 2 * 25 = 50;
                 with `add` in {-2..2} 52; with the epilogue v = sum * {1, 2} + {-3..3}: |v| <= 103
  other filters  taps in {-2, -1, 1, 2}, x / dz in {-1, 0, 1}: |sum| <= 2 * KH * KW <= 162 (9x9), 8x8: 128 (+3 with a shift)
  pyramid fwd    taps in {-1, 1}, x in {-2..2}: cumulative over four branches |sum| <= 4 * 9 * 2 = 72
  pyramid dx     dy in {-1, 0, 1} (|suffix sums| <= 4: exact in the bf16 gsum), taps in {-4..4} \\ {0}.  The worst case
                 9 * 4 * (4 + 3 + 2 + 1) = 360 is beyond the 256 up to which bf16 holds every integer; the seeded operands
                 stay below 128 (standard deviation 21), and check_exact asserts that the reference is representable
  weight grads   |x * dz| <= 4 (pyramid: |x * g| <= 2 * 4 = 8) over at most 17 000 pixels: < 2^18
  statistics     where P * max v^2 could reach 2^24 (the tiled shapes) x is sparse, 1 in 4 nonzero (1 in 8 leaves the 5-row map below half nonzero); sum v^2 < 2^24 is
                 asserted on the reference before the launch
Every exact reference has at least half of its elements nonzero (asserted), N >= 2 wherever a halo could reach the next
image, and the tiled cases are ragged in both directions against the kernel's tile (16 x 32, 8 x 32, 16 x 16).

RANDOM (`exact=False`): standard-normal operands rounded to their storage type, error = max|got - want| / max|want|:
  bf16 outputs                  2^-8     one rounding to an 8-bit significand (test_gather_ops.TOL_BF16 and its derivation)
  f32 outputs (forward, dx)     1e-5     sums of at most 81 products (test_gather_ops.TOL_F32)
  weight gradients, statistics  per element n * 2^-24 * S: the bound of an f32 sum of n terms in ANY order, S = the same
                                sum over the terms' absolute values (f64).  Weight gradient: the terms are x * dz over the
                                n = N * Ho * Wo pixels.  Statistics: v = scale * sum_t a_t + shift has taps + 1 terms and
                                one more rounding, v^2 their (taps + 2)^2 products: n = P * (taps + 2) resp. P * (taps + 2)^2,
                                S = sum_p u_p resp. sum_p u_p^2 with u_p = |scale| * sum_t |a_t| + |shift|.  Loose on purpose:
                                completeness is the exact cases' job.
Roundings of an intermediate that the reference models (nothing else is modelled):
  gsum = bf16(f32 running suffix sum of dy), once per stored value: pyr_suffix_kernel (csrc/backward.hip: `stv<V>(g + ...,
  run)` with T = bf16), read by pyr_bwd_data_kernel<bf16>, pyr_bwd_data_bf16_kernel, pyr_bwd_weight_kernel<bf16> and
  pyr_bwd_weight_bf16_kernel(from_dy = false); and pyr_bwd_data_ctx_kernel's own patch (its header comment in
  csrc/stencil_bf16.hip: "forms g_b ... in f32 and stores it rounded to bf16 -- bit for bit what pyr_suffix_kernel
  leaves in gsum").  pyr_bwd_data_tile_kernel (prefix-summed f32 filters), pyr_bwd_weight_same_kernel and
  pyr_bwd_weight_bf16_kernel(from_dy = true) keep their sums in f32: no rounding modelled.  With that one modelled
  rounding every bf16 family stays at the single output rounding 2^-8, except one:
  dw8x8_tile_kernel<1> + dw8x8_fold_kernel (dw8x8_bwd_data_tile, csrc/dwconv.hip) round twice: the gradient of the
  reflect-extended map goes to the workspace as bf16 (`d.y = scratch`, dtype_y = LEDN_BF16) and the fold adds up to four of
  those and `add` before it rounds the output.  Its bound is the sum of the two, 2 * 2^-8.

Not covered: dw3x3_tile_kernel<0,2,8> and <1,2,8>, which only the LEDN_DW_TH A/B knob selects (read once per process
under LEDN_EXPERIMENTAL).  dw8x8_wgrad_tile_kernel and the tiled forward statistics have one ending only (a partial row
per tile).  The issue's example "bf16 with C = 40" for dw_bwd_weight3x3_kernel<bf16,4> runs dw_bwd_weight_kernel<bf16,4>
(256 % (C / 4) != 0 declines there too: the id assertion found it); stride 2 and group_size 4 reach the instance.

The worst error per family and backend is printed when the module finishes (pytest -s)."""
import contextlib
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
OPT_STREAM_FAST, STREAM_FAST_DEFAULT = 2, 91
TOL_BF16, TOL_F32 = 2.0 ** -8, 1e-5
PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)]
DT_IDS = {F32: 'f32', BF16: 'bf16'}
ACTS = {None: 0, 'relu': 1, 'relu6': 2, 'prelu': 3, 'sigmoid': 4}

_WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    for (fam, dev), (err, bound, what) in sorted(_WORST.items()):
        print(f'\n[worst] {fam:34s} {dev:4s} err/bound {err:.3e}  (bound {bound})  at {what}', end='')
    print()


def rng(key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def gen(key, *shape):
    """seeded standard-normal f32 tensor; the seed is a digest of the case's key"""
    return torch.randn(*shape, generator=rng(key))


def q(t, dt):
    """values of t rounded to dt, kept in f32 (the reference promotes these to f64)"""
    return t.to(dt).float()


def ints(key, shape, lo, hi, keep=1.0, nonzero=False):
    """seeded integers in [lo, hi] (without 0 if nonzero); keep < 1 zeroes all but that share of the elements"""
    g = rng(key)
    vals = torch.tensor([v for v in range(lo, hi + 1) if v or not nonzero], dtype=torch.float32)
    t = vals[torch.randint(0, len(vals), shape, generator=g)]
    if keep < 1.0:
        t = t * (torch.rand(shape, generator=g) < keep)
    return t


def perm_taps(key, c):
    """[3, 3, c]: per channel a seeded permutation of the nine distinct values {-4..-1, 1..5}"""
    g = rng(key)
    vals = torch.tensor([-4., -3., -2., -1., 1., 2., 3., 4., 5.])
    return torch.stack([vals[torch.randperm(9, generator=g)] for _ in range(c)], 1).view(3, 3, c).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def dev_name(be):
    return 'emu' if be.dev.type == 'cpu' else 'hip'


def note(be, fam, err, bound, what):
    key = (fam, dev_name(be))
    if key not in _WORST or err > _WORST[key][0]:
        _WORST[key] = (err, bound, what)


def check_exact(be, fam, got, want, what, min_nonzero=0.5, nz_of=None):
    """got (device, any layout matching want) == want (f64) cast to got's type, bit for bit; names the first difference.
    nz_of: the tensor whose nonzero share guards against a vacuous pass (the pre-activation values where want went through
    a ReLU)"""
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nz = float(((want if nz_of is None else nz_of) != 0).double().mean())
    assert nz >= min_nonzero, f'{fam} {what}: only {nz:.2f} of the reference is nonzero: the case could pass vacuously'
    wt = want.to(got.dtype)
    assert torch.equal(wt.double(), want), f'{fam} {what}: the reference itself is not exact in {got.dtype}'
    note(be, fam + ' exact', 0.0 if torch.equal(got, wt) else 1.0, 'equality', what)
    if not torch.equal(got, wt):
        bad = (got != wt) | torch.isnan(got)
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f'{fam} {what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: '
                             f'got {float(got[idx])}, want {float(wt[idx])}')


def check_rel(be, fam, got, want, bound, what):
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f'{fam} {what}: non-finite output'
    err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
    note(be, fam, err / bound, f'{bound:.3e}', what)
    assert err <= bound, f'{fam} {what}: max|got-want|/max|want| = {err:.3e} > {bound:.3e}'


def check_sum(be, fam, got, want, n_terms, abs_sum, what):
    """|got - want| <= n * 2^-24 * S per element (an f32 sum of n terms in any order, S the sum of their absolute values)"""
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f'{fam} {what}: non-finite output'
    bound = n_terms * 2.0 ** -24 * abs_sum.double()
    ratio = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
    note(be, fam, ratio, 'n*2^-24*S', what)
    assert ratio <= 1.0, f'{fam} {what}: |got-want| = {ratio:.3e} x (n * 2^-24 * S), n = {n_terms}'


def out_tol(dt):
    return TOL_BF16 if dt == BF16 else TOL_F32


@contextlib.contextmanager
def stream_fast_bit1_cleared(on=True):
    """LEDN_OPT_STREAM_FAST without bit 1: the LDS-tiled kernels stand aside"""
    from led_net_amd import _lib
    lib = _lib.get_lib()
    if on:
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


# --------------------------------------------------------------------------- #
# references (float64, NCHW)
# --------------------------------------------------------------------------- #
def ref_dw(x, w, stride, pad, dil, gs, ext1):
    """x [N,C,H,W], w [KH,KW,C] -> depthwise conv, channel c with dilation dil[c // gs]; pad < 0: dil * (K - 1) // 2"""
    kh, kw, c = w.shape
    if ext1:
        x = F.pad(x, (0, 1, 0, 1), mode='reflect')
    outs = []
    for g in range((c + gs - 1) // gs):
        c0, c1 = g * gs, min(c, (g + 1) * gs)
        d = dil[g]
        ph = pad if pad >= 0 else d * (kh - 1) // 2
        pw = pad if pad >= 0 else d * (kw - 1) // 2
        outs.append(F.conv2d(x[:, c0:c1], w[:, :, c0:c1].permute(2, 0, 1)[:, None], stride=stride, padding=(ph, pw),
                             dilation=d, groups=c1 - c0))
    return torch.cat(outs, 1)


def ref_pyr_branches(x, w, dil, stride):
    """x [N,n,H,W], w [4,3,3,n] -> the four branch outputs (before the cumulative adds)"""
    n = x.shape[1]
    return [F.conv2d(x, w[b].permute(2, 0, 1)[:, None], stride=stride, padding=dil[b], dilation=dil[b], groups=n)
            for b in range(4)]


def act_ref(v, act, slope):
    if act == 'relu':
        return F.relu(v)
    if act == 'relu6':
        return F.relu6(v)
    if act == 'sigmoid':
        return torch.sigmoid(v)
    if act == 'prelu':
        return torch.where(v >= 0, v, v * slope.double().view(1, -1, 1, 1))
    return v


# --------------------------------------------------------------------------- #
# depthwise operands and references, cached per case (shared by the forward, the gradients and both backends)
# --------------------------------------------------------------------------- #
class Cfg:
    """geometry of one depthwise case; hashable"""

    def __init__(self, shape, k=(3, 3), stride=1, pad=-1, dil=(1, 1, 1, 1), gs=None, ext1=False):
        self.shape, self.k, self.stride, self.pad, self.dil, self.ext1 = tuple(shape), tuple(k), stride, pad, tuple(dil), ext1
        self.gs = gs or shape[3]

    def key(self):
        return (self.shape, self.k, self.stride, self.pad, self.dil, self.gs, self.ext1)

    def __hash__(self):
        return hash(self.key())

    def __eq__(self, o):
        return self.key() == o.key()

    def __repr__(self):
        n, h, w, c = self.shape
        return (f'{n}x{h}x{w}x{c} k{self.k[0]}x{self.k[1]} s{self.stride} pad{self.pad} dil{list(self.dil)} gs{self.gs}'
                + (' ext1' if self.ext1 else ''))

    def kw(self):
        return dict(stride=self.stride, pad=self.pad, dil=list(self.dil), group_size=self.gs, ext1=self.ext1)


@functools.lru_cache(maxsize=None)
def dw_operands(cfg, exact, dtx, sparse):
    """-> x [N,C,H,W] (values of dtx, f32), w [KH,KW,C] f32"""
    n, h, wd, c = cfg.shape
    if exact:
        k3 = cfg.k == (3, 3)
        w = perm_taps(('w', cfg.key()), c) if k3 else ints(('w', cfg.key()), (*cfg.k, c), -2, 2, nonzero=True)
        x = ints(('x', cfg.key()), (n, c, h, wd), *((-2, 2) if k3 else (-1, 1)), keep=0.25 if sparse else 1.0)
        return x, w
    scale = (cfg.k[0] * cfg.k[1]) ** -0.5
    return q(gen(('x', cfg.key()), n, c, h, wd), dtx), gen(('w', cfg.key()), *cfg.k, c) * scale


@functools.lru_cache(maxsize=None)
def dw_fwd_ref(cfg, exact, dtx, sparse):
    """-> y (pre-epilogue, f64), A = sum_t |x_t * w_t| per output (f64)"""
    x, w = dw_operands(cfg, exact, dtx, sparse)
    y = ref_dw(x.double(), w.double(), cfg.stride, cfg.pad, cfg.dil, cfg.gs, cfg.ext1)
    a = ref_dw(x.double().abs(), w.double().abs(), cfg.stride, cfg.pad, cfg.dil, cfg.gs, cfg.ext1)
    return y, a


def epilogue(cfg, exact, act):
    """-> scale, shift, slope [C] f32"""
    c = cfg.shape[3]
    if exact:
        k3 = cfg.k == (3, 3)
        scale = ints(('sc', cfg.key()), (c,), 1, 2) if k3 else torch.ones(c)
        return scale, ints(('sh', cfg.key()), (c,), -3, 3), None
    scale = gen(('sc', cfg.key()), c).abs() + 0.5
    slope = gen(('sl', cfg.key()), c).abs() * 0.3 if act == 'prelu' else None
    return scale, gen(('sh', cfg.key()), c), slope


def need_sparse(cfg):
    """the exact statistics of this shape need a sparse x: P * max v^2 could reach 2^24 otherwise"""
    n, h, w, _ = cfg.shape
    vmax = 103 if cfg.k == (3, 3) else 2 * cfg.k[0] * cfg.k[1] + 3
    return n * (h + 1) * (w + 1) * vmax * vmax >= 2 ** 24


def run_dw_fwd(be, expect, cfg, *, pair=(BF16, BF16), epi=False, act=None, stats=False, exact=True, det=False,
               sf_clear=False):
    """one ledn_dwconv2d launch against the reference; expect = kernel_name of the instance (with its ending)"""
    from led_net_amd import ops
    dtx, dty = pair
    sparse = stats and exact and need_sparse(cfg)
    x, w = dw_operands(cfg, exact, dtx, sparse)
    y, a = dw_fwd_ref(cfg, exact, dtx, sparse)
    c, taps = cfg.shape[3], cfg.k[0] * cfg.k[1]
    scale = shift = slope = None
    v = y
    if epi:
        scale, shift, slope = epilogue(cfg, exact, act)
        v = y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    want = act_ref(v, act, slope)
    what = f'{cfg} {DT_IDS[dtx]}->{DT_IDS[dty]} epi={epi} act={act} stats={stats} det={det}'
    if exact and stats:
        assert float((v * v).sum((0, 2, 3)).max()) < 2 ** 24, f'{what}: sum v^2 leaves the exact range of f32'
    st = (torch.zeros(c), torch.zeros(c)) if stats else None
    kw = dict(cfg.kw(), out_scale=be(scale), out_shift=be(shift), act=ACTS[act], slope=be(slope),
              stats=tuple(be(s) for s in st) if stats else None, out_dtype=dty)
    xd, wd = be(nhwc(x).to(dtx)), be(w)
    with stream_fast_bit1_cleared(sf_clear), deterministic(det):
        name = ops.kernel_name(ops.DW_KERNELS, ops.dwconv2d_kernel_id(xd, wd, **kw))
        assert name == expect, f'{what}: runs on {name}, written for {expect}'
        got = ops.dwconv2d(xd, wd, **kw)
    assert got.dtype == dty
    fam = expect.split('+')[0] + f' ->{DT_IDS[dty]}'
    if exact:
        check_exact(be, fam, nchw(got), want, what, nz_of=v)
        if stats:
            check_exact(be, expect + ' stat', kw['stats'][0], v.sum((0, 2, 3)), what + ' sum')
            check_exact(be, expect + ' stat', kw['stats'][1], (v * v).sum((0, 2, 3)), what + ' sqsum')
        return
    check_rel(be, fam, nchw(got), want, out_tol(dty), what)
    if stats:
        u = a if not epi else a * scale.double().abs().view(1, -1, 1, 1) + shift.double().abs().view(1, -1, 1, 1)
        p = v.numel() // c
        check_sum(be, expect + ' stat', kw['stats'][0], v.sum((0, 2, 3)), p * (taps + 2), u.sum((0, 2, 3)), what + ' sum')
        check_sum(be, expect + ' stat', kw['stats'][1], (v * v).sum((0, 2, 3)), p * (taps + 2) ** 2, (u * u).sum((0, 2, 3)),
                  what + ' sqsum')


@functools.lru_cache(maxsize=None)
def dw_bwd_ref(cfg, exact, dt):
    """-> x, w, dz, dx (without add), dw, S = sum_p |x_tap * dz| per filter element"""
    x, w = dw_operands(cfg, exact, dt, False)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = ref_dw(xr, wr, cfg.stride, cfg.pad, cfg.dil, cfg.gs, cfg.ext1)
    k3 = cfg.k == (3, 3)
    dz = ints(('dz', cfg.key()), tuple(y.shape), *((-2, 2) if k3 else (-1, 1))) if exact else q(gen(('dz', cfg.key()), *y.shape), dt)
    dx, dw = torch.autograd.grad(y, (xr, wr), dz.double())
    xa = x.double().abs().requires_grad_(True)
    wa = w.double().abs().requires_grad_(True)
    s, = torch.autograd.grad(ref_dw(xa, wa, cfg.stride, cfg.pad, cfg.dil, cfg.gs, cfg.ext1), (wa,), dz.double().abs())
    return x, w, dz, dx.detach(), dw.detach(), s.detach()


def run_dw_bwd(be, expect_data, expect_weight, cfg, *, dt=BF16, exact=True, det=False, sf_clear=False, fused=None):
    """data gradient with and without `add`, weight gradient into zeros and into a non-zero dw_out (separate entries),
    and -- fused is not None -- ledn_dwconv2d_bwd; expect_* = kernel_name of the instance (None: not run here)"""
    from led_net_amd import ops, ops_train as T
    x, w, dz, dx, dw, s = dw_bwd_ref(cfg, exact, dt)
    xd, dzd, wd = be(nhwc(x).to(dt)), be(nhwc(dz).to(dt)), be(w)
    add = ints(('add', cfg.key()), tuple(x.shape), -2, 2) if exact else q(gen(('add', cfg.key()), *x.shape), dt)
    addd = be(nhwc(add).to(dt))
    dw0 = ints(('dw0', cfg.key()), tuple(w.shape), -9, 9) if exact else gen(('dw0', cfg.key()), *w.shape)
    npix = dz.shape[0] * dz.shape[2] * dz.shape[3]
    what = f'{cfg} {DT_IDS[dt]} det={det}'
    with stream_fast_bit1_cleared(sf_clear), deterministic(det):
        kd, kwt = T.dwconv2d_bwd_kernel_ids(xd, dzd, wd, **cfg.kw())
        nd, nw = ops.kernel_name(T.DW_BWD_DATA_KERNELS, kd), ops.kernel_name(T.DW_BWD_WEIGHT_KERNELS, kwt)
        if fused is not None:
            assert T.dwconv2d_bwd_fused_applies(xd, dzd, wd, **cfg.kw()) == fused, what
        if expect_data is not None:
            assert nd == expect_data, f'{what}: data gradient runs on {nd}, written for {expect_data}'
            for with_add in (False, True):
                got, _ = T.dwconv2d_bwd(xd, dzd, wd, **cfg.kw(), add=addd if with_add else None, need_dw=False)
                want = dx + add.double() if with_add else dx
                fam = f'{expect_data} {DT_IDS[dt]}'
                if exact:
                    check_exact(be, fam, nchw(got), want, f'{what} add={with_add}')
                else:
                    tol = 2 * TOL_BF16 if expect_data == 'dw8x8_tile_kernel<1>' else out_tol(dt)      # two roundings: docstring
                    check_rel(be, fam, nchw(got), want, tol, f'{what} add={with_add}')
        if expect_weight is not None:
            assert nw == expect_weight, f'{what}: weight gradient runs on {nw}, written for {expect_weight}'
            for init in (False, True):
                sink = be(dw0.clone()) if init else None
                _, got = T.dwconv2d_bwd(xd, dzd, wd, **cfg.kw(), need_dx=False, dw_out=sink)
                want = dw + dw0.double() if init else dw
                if exact:
                    check_exact(be, expect_weight, got, want, f'{what} dw_out={init}', min_nonzero=0.4)
                else:
                    check_sum(be, expect_weight, got, want, npix + 1, s + dw0.double().abs() * init, f'{what} dw_out={init}')
        if fused:
            got_dx, got_dw = T.dwconv2d_bwd(xd, dzd, wd, **cfg.kw(), add=addd, dw_out=be(dw0.clone()))
            if exact:
                check_exact(be, 'dw3x3_bwd_tile_kernel dx', nchw(got_dx), dx + add.double(), what)
                check_exact(be, 'dw3x3_bwd_tile_kernel dw', got_dw, dw + dw0.double(), what, min_nonzero=0.4)
            else:
                check_rel(be, 'dw3x3_bwd_tile_kernel dx', nchw(got_dx), dx + add.double(), TOL_BF16, what)
                check_sum(be, 'dw3x3_bwd_tile_kernel dw', got_dw, dw + dw0.double(), npix + 1, s + dw0.double().abs(), what)


# --------------------------------------------------------------------------- #
# 1. forward, the LDS-tiled and vectorised bf16 instances
# --------------------------------------------------------------------------- #
T8 = Cfg((2, 45, 47, 32), k=(8, 8), pad=3, ext1=True)                      # ragged against 8 x 32
T216 = Cfg((2, 91, 93, 32), dil=(1, 2, 2, 1), gs=8)                       # ragged against 16 x 32
T58 = Cfg((2, 83, 101, 32), dil=(2, 3, 4, 5), gs=8)                       # ragged against 8 x 32, one slice = four dilations
T58_LOW = Cfg((1, 5, 3300, 32), dil=(2, 3, 4, 5), gs=8)                   # a map lower than one tile
T_DIL6 = Cfg((2, 91, 93, 32), dil=(6, 1, 2, 3), gs=8)                     # halo beyond the tile kernel's 5
SMALL32 = Cfg((3, 13, 21, 32), dil=(1, 2, 3, 1), gs=8)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
def test_dw8x8_tile_forward(be, exact):
    run_dw_fwd(be, 'dw8x8_tile_kernel<0>', T8, exact=exact)
    run_dw_fwd(be, 'dw8x8_tile_kernel<0>+partial', T8, stats=True, exact=exact)
    run_dw_fwd(be, 'dw8x8_tile_kernel<0>+partial', T8, stats=True, epi=True, act='relu', exact=exact)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
def test_dw3x3_tile_forward(be, exact):
    for cfg, plain, epi in ((T216, 'dw3x3_tile_kernel<0,2,16,false>', 'dw3x3_tile_kernel<0,2,16>'),
                            (T58, 'dw3x3_tile_kernel<0,5,8,false>', 'dw3x3_tile_kernel<0,5,8>'),
                            (T58_LOW, 'dw3x3_tile_kernel<0,5,8,false>', 'dw3x3_tile_kernel<0,5,8>')):
        run_dw_fwd(be, plain, cfg, exact=exact)
        run_dw_fwd(be, plain + '+partial', cfg, stats=True, exact=exact)
        run_dw_fwd(be, epi + '+partial', cfg, stats=True, epi=True, act='relu', exact=exact)
    if not exact:
        run_dw_fwd(be, 'dw3x3_tile_kernel<0,2,16>', T216, epi=True, act='prelu', exact=False)
        run_dw_fwd(be, 'dw3x3_tile_kernel<0,5,8>', T58, epi=True, act='relu6', exact=False)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
def test_dw3x3_bf16_forward(be, exact):
    k = 'dw3x3_bf16_kernel<0>'
    run_dw_fwd(be, k, SMALL32, exact=exact)
    run_dw_fwd(be, k + '+atomic', SMALL32, stats=True, exact=exact)                     # 4 workgroups
    run_dw_fwd(be, k + '+partial', SMALL32, stats=True, exact=exact, det=True)
    run_dw_fwd(be, k + '+atomic', SMALL32, stats=True, epi=True, act='relu', exact=exact)
    run_dw_fwd(be, k, T216, exact=exact, sf_clear=True)
    run_dw_fwd(be, k + '+partial', T216, stats=True, exact=exact, sf_clear=True)        # 265 workgroups
    run_dw_fwd(be, k, T_DIL6, exact=exact)
    run_dw_fwd(be, k + '+partial', T_DIL6, stats=True, epi=True, act='relu', exact=exact)
    if not exact:
        run_dw_fwd(be, k, SMALL32, epi=True, act='prelu', exact=False)
        run_dw_fwd(be, k, SMALL32, epi=True, act='relu6', exact=False)


# --------------------------------------------------------------------------- #
# 2. forward, the generic kernel: V in {4 (3x3), 4, 1} x four dtype pairs
# --------------------------------------------------------------------------- #
def small(c, **kw):
    return Cfg((2, 11, 13, c), **kw)


V1, V4, V43 = 'dwconv_kernel<1,0>', 'dwconv_kernel<4,0>', 'dwconv_kernel<4,9>'
# (instance, geometry).  bf16 -> bf16 with C % 8 == 0, group_size % 8 == 0, 256 % (C / 8) == 0, 3x3, stride 1, no ext1 and
# pad < 0 or = dil belongs to dw3x3_bf16_kernel: every 3x3 line below with C in {8, 40} breaks one of those conditions
GENERIC = [
    (V1, small(5)), (V1, small(5, k=(5, 3), stride=2)), (V1, small(5, k=(2, 2), ext1=True)),
    (V1, small(6, gs=3, dil=(1, 2, 1, 1))), (V1, small(6, gs=3, k=(9, 9), dil=(1, 1, 1, 1), pad=0, ext1=True)),
    (V1, small(6, gs=3, k=(3, 8), stride=2)), (V1, small(6, gs=3, dil=(3, 3, 3, 3), pad=1, stride=2, ext1=True)),
    (V1, small(5, k=(8, 8), pad=3, ext1=True)),
    (V43, small(12, gs=8, dil=(1, 3, 1, 1))), (V43, small(12, gs=8, dil=(2, 2, 2, 2), pad=1)),
    (V43, small(12, gs=8, dil=(2, 1, 1, 1), ext1=True)), (V43, small(12, gs=8, dil=(3, 2, 1, 1), stride=2)),
    (V43, small(8, stride=2)), (V43, small(8, ext1=True)), (V43, small(8, dil=(2, 2, 2, 2), pad=0)),
    (V43, small(24, gs=8, dil=(1, 2, 3, 1))), (V43, small(24, gs=8, dil=(3, 3, 3, 3), pad=2, stride=2, ext1=True)),
    (V43, small(40, gs=20, dil=(2, 1, 1, 1))),
    (V4, small(12, gs=8, k=(5, 3), dil=(1, 2, 1, 1))), (V4, small(12, gs=8, k=(2, 2), stride=2)),
    (V4, small(8, k=(3, 8))), (V4, small(8, k=(3, 8), stride=2, pad=0, ext1=True)),
    (V4, small(8, k=(9, 9), dil=(1, 1, 1, 1))), (V4, small(24, gs=8, k=(9, 9), dil=(1, 1, 1, 1), pad=2, stride=2)),
    (V4, small(8, k=(8, 8), pad=3, ext1=True)), (V4, small(40, gs=20, k=(8, 8), pad=3, ext1=True, stride=2)),
    (V4, small(40, gs=20, k=(5, 3), dil=(1, 2, 1, 1), ext1=True)), (V4, small(24, gs=8, k=(2, 2), pad=1)),
]


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
@pytest.mark.parametrize('pair', PAIRS, ids=['f32-f32', 'bf16-bf16', 'bf16-f32', 'f32-bf16'])
def test_dwconv_generic_forward(be, pair, exact):
    for i, (k, cfg) in enumerate(GENERIC):
        run_dw_fwd(be, k, cfg, pair=pair, exact=exact)
        if i % 3 == 0:                                                            # 1 or 2 workgroups: atomics
            run_dw_fwd(be, k + '+atomic', cfg, pair=pair, stats=True, epi=cfg.k == (3, 3), act='relu', exact=exact)
        if i % 3 == 1:
            run_dw_fwd(be, k + '+partial', cfg, pair=pair, stats=True, exact=exact, det=True)
    if not exact:
        for k, cfg in (GENERIC[0], GENERIC[8], GENERIC[18]):
            for act in ('sigmoid', 'prelu', 'relu6'):
                run_dw_fwd(be, k, cfg, pair=pair, epi=True, act=act, exact=False)


# --------------------------------------------------------------------------- #
# 3. data gradient
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
def test_dw_bwd_data_tiled(be, exact):
    run_dw_bwd(be, 'dw8x8_tile_kernel<1>', None, T8, exact=exact)
    run_dw_bwd(be, 'dw3x3_tile_kernel<1,2,16>', None, T216, exact=exact)
    run_dw_bwd(be, 'dw3x3_tile_kernel<1,5,8>', None, T58, exact=exact)
    run_dw_bwd(be, 'dw3x3_tile_kernel<1,5,8>', None, T58_LOW, exact=exact)
    run_dw_bwd(be, 'dw3x3_bf16_kernel<1>', None, SMALL32, exact=exact)
    run_dw_bwd(be, 'dw3x3_bf16_kernel<1>', None, T216, exact=exact, sf_clear=True)
    run_dw_bwd(be, 'dw3x3_bf16_kernel<1>', None, T_DIL6, exact=exact)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_dw_bwd_data_generic(be, dt, exact):
    """the general path (even filters at stride 2, ext1 with 3x3 and 8x8) and the 3x3 path of dw_bwd_data_kernel<T,4|1>"""
    for k, cfg in GENERIC:
        run_dw_bwd(be, 'dw_bwd_data_kernel<1>' if k == V1 else 'dw_bwd_data_kernel<4>', None, cfg, dt=dt, exact=exact)


# --------------------------------------------------------------------------- #
# 4. weight gradient: every kernel with both endings (atomic in default mode on these small grids, partial rows in
#    deterministic mode), into zeros and into a non-zero dw_out
# --------------------------------------------------------------------------- #
TAP1, TAP4, ROW, W33, WBF = ('dw_bwd_weight_kernel<1>', 'dw_bwd_weight_kernel<4>', 'dw_bwd_weight_row_kernel<4,8>',
                             'dw_bwd_weight3x3_kernel<4>', 'dw3x3_bwd_weight_bf16_kernel')
WGRAD = [
    (F32, TAP1, small(5)), (BF16, TAP1, small(6, gs=3, dil=(1, 2, 1, 1))), (BF16, TAP1, small(5, k=(2, 2), stride=2, ext1=True)),
    (F32, TAP4, small(12, gs=8, dil=(1, 3, 1, 1))), (BF16, TAP4, small(24, gs=8, dil=(1, 2, 3, 1))),       # 256 % (C / 4) != 0
    (BF16, TAP4, small(40, gs=20, dil=(2, 1, 1, 1))), (F32, TAP4, small(8, k=(5, 3), stride=2)),
    (BF16, TAP4, small(8, ext1=True)),                                                                    # ext1 declines 3x3
    (F32, ROW, small(8, k=(8, 8), pad=3, ext1=True)), (BF16, ROW, small(8, k=(8, 8), pad=3, ext1=True, stride=2)),
    (BF16, ROW, small(8, k=(3, 8))), (F32, ROW, small(16, gs=4, k=(3, 8), stride=2, pad=0, ext1=True)),
    (F32, W33, small(8, dil=(2, 2, 2, 2))), (F32, W33, small(16, gs=4, dil=(1, 2, 3, 1), stride=2)),
    (BF16, W33, small(8, stride=2)), (BF16, W33, small(16, gs=4, dil=(1, 2, 3, 1))), (BF16, W33, small(8, dil=(2, 2, 2, 2), pad=1)),
    (BF16, WBF, small(8, dil=(2, 2, 2, 2))), (BF16, WBF, SMALL32),
]


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'partial'])
def test_dw_bwd_weight(be, det, exact):
    end = '+partial' if det else '+atomic'
    for dt, k, cfg in WGRAD:
        run_dw_bwd(be, None, k + end, cfg, dt=dt, exact=exact, det=det)
    run_dw_bwd(be, None, WBF + end, T216, exact=exact, det=det)                      # 17 workgroups
    run_dw_bwd(be, None, WBF + end, T58, exact=exact, det=det)
    run_dw_bwd(be, None, 'dw8x8_wgrad_tile_kernel+partial', T8, exact=exact, det=det)


# --------------------------------------------------------------------------- #
# 5. both gradients in one launch (dw3x3_bwd_tile_kernel<2,16> and <5,8>; tests/test_dw_bwd_fused.py keeps its own checks)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
def test_dw_bwd_fused_instances(be, exact):
    run_dw_bwd(be, None, None, T216, exact=exact, fused=True)
    run_dw_bwd(be, None, None, T58, exact=exact, fused=True)
    run_dw_bwd(be, None, None, T_DIL6, exact=exact, fused=False)       # the gate's dilation limit, asserted only


# --------------------------------------------------------------------------- #
# 6. SESP pyramid
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def pyr_ref(shape, dil, stride, exact, dt, model_gsum):
    """-> x [N,n,H,W], w [4,3,3,n], wb (taps of the gradient cases), y, dy, dx, dw, S (dw's absolute-value sum)
    forward operands: w in {-1, 1}; gradient operands: wb in {-4..4} \\ {0}, dy in {-1, 0, 1}"""
    n_, h, wd, n = shape
    key = (shape, dil, stride)
    if exact:
        x = ints(('px', key), (n_, n, h, wd), -2, 2)
        w = ints(('pw', key), (4, 3, 3, n), -1, 1, nonzero=True)
        wb = ints(('pwb', key), (4, 3, 3, n), -4, 4, nonzero=True)
    else:
        x = q(gen(('px', key), n_, n, h, wd), dt)
        w = gen(('pw', key), 4, 3, 3, n) / 3
        wb = gen(('pwb', key), 4, 3, 3, n) / 3
    outs = ref_pyr_branches(x.double(), w.double(), dil, stride)
    y = torch.cat([sum(outs[:b + 1]) for b in range(4)], 1)
    dy = ints(('pdy', key), tuple(y.shape), -1, 1) if exact else q(gen(('pdy', key), *y.shape), dt)
    # suffix sums g_b = sum_{b' >= b} dy_b'; model_gsum: each stored value is bf16 of the f32 running sum
    g, run = [None] * 4, torch.zeros(n_, n, *y.shape[2:])
    for b in (3, 2, 1, 0):
        run = run + dy[:, b * n:(b + 1) * n]
        g[b] = (run.to(BF16).float() if model_gsum else run).double()
    xr, wr = x.double().requires_grad_(True), wb.double().requires_grad_(True)
    br = ref_pyr_branches(xr, wr, dil, stride)
    dx, dw = torch.autograd.grad(br, (xr, wr), g)
    xa, wa = x.double().abs().requires_grad_(True), wb.double().abs().requires_grad_(True)
    s, = torch.autograd.grad(ref_pyr_branches(xa, wa, dil, stride), (wa,), [t.abs() for t in g])
    return x, w, wb, y, dy, dx.detach(), dw.detach(), s.detach()


def run_pyr_fwd(be, expect, shape, dil, stride, dt, exact):
    from led_net_amd import ops
    x, w, _, y, *_ = pyr_ref(shape, tuple(dil), stride, exact, dt, False)
    xd, wd = be(nhwc(x).to(dt)), be(w)
    what = f'{shape} dil{list(dil)} s{stride} {DT_IDS[dt]}'
    name = ops.PYR_KERNELS[ops.sesp_pyramid_kernel_id(xd, wd, list(dil), stride)]
    assert name == expect, f'{what}: runs on {name}, written for {expect}'
    got = ops.sesp_pyramid(xd, wd, list(dil), stride)
    fam = f'{expect} {DT_IDS[dt]}'
    if exact:
        check_exact(be, fam, nchw(got), y, what)
    else:
        check_rel(be, fam, nchw(got), y, out_tol(dt), what)


DILS = [(1, 2, 3, 4), (4, 1, 3, 2), (2, 2, 2, 2)]


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
def test_sesp_pyramid_forward(be, exact):
    for stride in (1, 2):
        for dil in DILS:
            same = len(set(dil)) == 1
            for n in (8, 32):
                run_pyr_fwd(be, 'pyr_fwd_bf16_kernel<true>' if same else 'pyr_fwd_bf16_kernel<false>', (2, 13, 11, n), dil,
                            stride, BF16, exact)
            for n in (4, 6, 8, 24):
                v = 'sesp_pyramid_kernel<4>' if n % 4 == 0 else 'sesp_pyramid_kernel<1>'
                run_pyr_fwd(be, v, (2, 13, 11, n), dil, stride, F32, exact)
                if n != 8:                 # bf16 with n = 8 belongs to pyr_fwd_bf16_kernel; 256 % (24 / 8) != 0 declines
                    run_pyr_fwd(be, v, (2, 13, 11, n), dil, stride, BF16, exact)


def run_pyr_bwd(be, kid_data, expect_weight, shape, dil, stride, dt, exact, det=False, sf_clear=False):
    from led_net_amd import ops, ops_train as T
    model = dt == BF16 and kid_data in (0, 1, 3)
    x, _, wb, y, dy, dx, dw, s = pyr_ref(shape, tuple(dil), stride, exact, dt, model)
    if dt == BF16 and kid_data in (0, 1, 3) and expect_weight.startswith('pyr_bwd_weight_bf16_kernel<from_dy>'):
        # the data gradient reads the rounded suffix sums, this weight gradient forms its own in f32
        dw, s = pyr_ref(shape, tuple(dil), stride, exact, dt, False)[6:8]
    xd, dyd, wd = be(nhwc(x).to(dt)), be(nhwc(dy).to(dt)), be(wb)
    dw0 = ints(('pdw0', shape, dil), tuple(wb.shape), -9, 9) if exact else gen(('pdw0', shape, dil), *wb.shape)
    what = f'{shape} dil{list(dil)} s{stride} {DT_IDS[dt]} det={det}'
    npix = dy.shape[0] * dy.shape[2] * dy.shape[3]
    with stream_fast_bit1_cleared(sf_clear), deterministic(det):
        kd = T.sesp_pyramid_bwd_kernel_id(xd, dyd, list(dil), stride)
        assert kd == kid_data, f'{what}: data gradient runs on {T.PYR_BWD_KERNELS[kd]}, written for {T.PYR_BWD_KERNELS[kid_data]}'
        nw = ops.kernel_name(T.PYR_BWD_WEIGHT_KERNELS, T.sesp_pyramid_bwd_weight_kernel_id(xd, dyd, list(dil), stride))
        assert nw == expect_weight, f'{what}: weight gradient runs on {nw}, written for {expect_weight}'
        for init in (False, True):
            got_dx, got_dw = T.sesp_pyramid_bwd(xd, dyd, wd, list(dil), stride, dw_out=be(dw0.clone()) if init else None)
            want_dw = dw + dw0.double() if init else dw
            fam = f'{T.PYR_BWD_KERNELS[kid_data]} {DT_IDS[dt]}'
            if exact:
                check_exact(be, fam, nchw(got_dx), dx, what)
                check_exact(be, expect_weight, got_dw, want_dw, f'{what} dw_out={init}', min_nonzero=0.4)
            else:
                check_rel(be, fam, nchw(got_dx), dx, out_tol(dt), what)
                check_sum(be, expect_weight, got_dw, want_dw, npix + 1, s + dw0.double().abs() * init, f'{what} dw_out={init}')


PW1, PW4, PWB, PWD, PWS = ('pyr_bwd_weight_kernel<1>', 'pyr_bwd_weight_kernel<4>', 'pyr_bwd_weight_bf16_kernel',
                           'pyr_bwd_weight_bf16_kernel<from_dy>', 'pyr_bwd_weight_same_kernel')
S13 = (2, 13, 11)
S21 = (2, 21, 19)                                                                    # ragged against PYC_T = 16
# (data-gradient id, weight-gradient instance, shape, dilations, stride, dtype).  At stride 2 an all-even dilation leaves three
# of four dx pixels structurally zero (below the nonzero share an exact case needs): odd or mixed dilations there
PYR_BWD = [
    (0, PW4, (*S13, 8), (1, 2, 3, 4), 1, F32), (0, PW4, (*S13, 8), (4, 1, 3, 2), 2, F32), (0, PW1, (*S13, 6), (1, 2, 3, 4), 1, F32),
    (0, PW1, (*S13, 6), (3, 3, 3, 3), 2, F32), (0, PW4, (*S13, 4), (1, 2, 3, 4), 1, BF16), (0, PW4, (*S13, 4), (1, 2, 3, 4), 2, BF16),
    (0, PW1, (*S13, 6), (1, 2, 3, 4), 1, BF16), (0, PW1, (*S13, 6), (4, 1, 3, 2), 2, BF16),
    (0, PW4, (*S13, 24), (1, 2, 3, 4), 1, BF16),                                     # n / 8 = 3: no vectorised kernel takes it
    (0, PWB, (*S13, 8), (1, 2, 3, 9), 2, BF16),                                      # halo 5 at stride 2: neither ctx nor id 1
    (1, PWB, (*S13, 8), (1, 2, 3, 9), 1, BF16), (1, PWB, (*S13, 64), (1, 2, 3, 9), 1, BF16),
    (3, PWD, (*S21, 8), (1, 2, 3, 4), 1, BF16), (3, PWD, (*S21, 8), (1, 2, 3, 4), 2, BF16),
    (3, PWD, (*S21, 16), (4, 1, 3, 2), 1, BF16), (3, PWD, (*S21, 16), (1, 2, 3, 4), 2, BF16),
    (3, PWD, (*S21, 16), (1, 1, 1, 1), 1, BF16),                                     # equal dilations below the tile kernel's size
]


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'partial'])
def test_sesp_pyramid_bwd_small(be, det, exact):
    end = '+partial' if det else '+atomic'
    for kd, kw, shape, dil, stride, dt in PYR_BWD:
        run_pyr_bwd(be, kd, kw + end, shape, dil, stride, dt, exact, det=det)


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'random'])
@pytest.mark.parametrize('det', [False, True], ids=['atomic', 'partial'])
def test_sesp_pyramid_bwd_tile(be, det, exact):
    """pyr_bwd_data_tile_kernel with pyr_bwd_weight_same_kernel (n <= 64) and with the from_dy gather (n = 128)"""
    # 67 workgroups: partial rows in either mode (the gate's 16384 pixels are beyond the 32 workgroups that end in atomics)
    run_pyr_bwd(be, 2, PWS + '+partial', (2, 91, 93, 16), (1, 1, 1, 1), 1, BF16, exact, det=det)
    if not det:
        run_pyr_bwd(be, 2, PWD + '+partial', (2, 91, 93, 128), (1, 1, 1, 1), 1, BF16, exact)     # 133 workgroups: partial rows
        run_pyr_bwd(be, 1, PWB + '+atomic', (2, 91, 93, 16), (1, 1, 1, 1), 1, BF16, exact, sf_clear=True)


# --------------------------------------------------------------------------- #
# 7. filter-bank repack: pure permutations, arbitrary floats, equality
# --------------------------------------------------------------------------- #
def packed_ref(ws, stacked):
    """[n_k,1,KH,KW] filters -> [K,KH,KW,n] (stacked) or [KH,KW,sum n] by plain indexing"""
    per = [w[:, 0].permute(1, 2, 0) for w in ws]
    return torch.stack(per) if stacked else torch.cat(per, 2)


def unpacked_ref(dpacked, ws, stacked):
    if stacked:
        return [dpacked[k].permute(2, 0, 1)[:, None] for k in range(len(ws))]
    out, c0 = [], 0
    for w in ws:
        out.append(dpacked[:, :, c0:c0 + w.shape[0]].permute(2, 0, 1)[:, None])
        c0 += w.shape[0]
    return out


BANKS = [([8, 8, 8, 8], (3, 3), True), ([5, 12, 7], (3, 3), False), ([32], (8, 8), False), ([6, 6], (8, 8), True),
         ([3, 1, 40, 2, 9, 4, 4, 16], (3, 3), False), ([300], (3, 3), False)]      # 8 sources; more than one 256-lane trip


def test_dw_pack_and_unpack_grad(be):
    from led_net_amd import ops_train as T
    for ns, k, stacked in BANKS:
        ws = [gen(('bank', tuple(ns), k, i), n, 1, *k) for i, n in enumerate(ns)]
        got = T.dw_pack([be(w) for w in ws], stacked)
        want = packed_ref(ws, stacked)
        assert torch.equal(got.cpu(), want), (ns, k, stacked)
        dpacked = gen(('dbank', tuple(ns), k), *want.shape)
        sinks0 = [gen(('sink', tuple(ns), k, i), *w.shape) for i, w in enumerate(ws)]
        sinks = [be(s.clone()) for s in sinks0]
        T.dw_unpack_grad([be(w) for w in ws], sinks, be(dpacked), stacked)
        for s, s0, d in zip(sinks, sinks0, unpacked_ref(dpacked, ws, stacked)):
            assert torch.equal(s.cpu(), s0 + d), (ns, k, stacked)


def test_dw_repack_multi(be):
    """direction 0 packs every bank; direction 1 adds the packed gradients into the sinks AND re-zeroes them"""
    from led_net_amd import ops_train as T
    banks, host = [], []
    for ns, k, stacked in BANKS:
        ws = [gen(('mbank', tuple(ns), k, i), n, 1, *k) for i, n in enumerate(ns)]
        want = packed_ref(ws, stacked)
        sinks0 = [gen(('msink', tuple(ns), k, i), *w.shape) for i, w in enumerate(ws)]
        dp0 = gen(('mdbank', tuple(ns), k), *want.shape)
        packed = be(torch.full(want.shape, float('nan')))
        banks.append(([be(w) for w in ws], [be(s.clone()) for s in sinks0], stacked, packed, be(dp0.clone())))
        host.append((ws, want, sinks0, dp0))
    table = T.DwBankTable(banks)
    table.run(0)
    for (ws, want, sinks0, dp0), (_, sinks, stacked, packed, dpacked) in zip(host, banks):
        assert torch.equal(packed.cpu(), want)
        assert torch.equal(dpacked.cpu(), dp0), 'direction 0 touched the packed gradient'
        assert all(torch.equal(s.cpu(), s0) for s, s0 in zip(sinks, sinks0)), 'direction 0 touched a gradient sink'
    table.run(1)
    for (ws, want, sinks0, dp0), (_, sinks, stacked, packed, dpacked) in zip(host, banks):
        for s, s0, d in zip(sinks, sinks0, unpacked_ref(dp0, ws, stacked)):
            assert torch.equal(s.cpu(), s0 + d)
        assert torch.equal(dpacked.cpu(), torch.zeros_like(dp0)), 'direction 1 left the packed gradient behind'
        assert torch.equal(packed.cpu(), want), 'direction 1 touched the packed filters'
    table.run(1)                                                    # a second flush adds nothing
    for (ws, want, sinks0, dp0), (_, sinks, stacked, packed, dpacked) in zip(host, banks):
        for s, s0, d in zip(sinks, sinks0, unpacked_ref(dp0, ws, stacked)):
            assert torch.equal(s.cpu(), s0 + d)
