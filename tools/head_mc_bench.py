#!/usr/bin/env python3
"""The multi-class head kernels (csrc/head_mc.hip) against the generic kernels they replace, on the MI355X: forward, data
gradient and weight gradient of LEDHead's head_x1 / head_x2 convolution (norm -> ReLU -> conv3x3, 32 -> Co) at
16 x 512 x 512 x 32 and 16 x 256 x 256 x 32 for Co in {11, 19, 32}, with LEDN_HEAD_MC=1 and =0 -- each setting in a fresh
child process (the knob is read once) -- and the two-class kernels at Co = 2 as the floor.  HIP events around each call,
median of --repeats after --warmup, device synchronised before and after a series.  GB/s: the bytes a call must move at
least (x or dz read once, the output written once) over the median time.

    python tools/head_mc_bench.py [--out profiles/head_mc_bench.txt]
"""
import argparse
import os
import os.path as osp
import statistics
import subprocess
import sys

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)

FWD = ('conv_direct_kernel', 'conv_mfma_kernel', 'conv1x1_mfma_kernel', 'conv3x3_reg_kernel', 'conv3x3_narrowin_mfma_kernel',
       'conv_f32_mfma_kernel', 'head_fwd_kernel', 'head_mc_fwd_kernel', 'head_mc_dgrad_kernel')
WG = ('conv_wgrad_direct', 'conv_wgrad_mfma_kernel', 'conv3x3_wgrad_narrow_kernel', 'conv1x1_wgrad_reg_kernel',
      'conv_wgrad_f32_mfma_kernel', 'head_mc_wgrad_kernel')


def timed(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    return statistics.median(ms), min(ms), max(ms)


def child(a):
    import torch
    from led_net_amd import ops
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(304)
    for (N, H, W) in ((16, 512, 512), (16, 256, 256)):
        x = torch.randn(N, H, W, 32, generator=g).bfloat16().to(dev)
        sc, sh = (torch.rand(32, generator=g) + 0.5).to(dev), (torch.randn(32, generator=g) * 0.3).to(dev)
        for co in a.classes:
            w = (torch.randn(co, 32, 3, 3, generator=g) / 17.0).to(dev)
            dz = torch.randn(N, H, W, co, generator=g).bfloat16().to(dev)
            sink = torch.zeros(co, 32, 3, 3, device=dev)
            kw = dict(pad=1, in_scale=sc, in_shift=sh, in_act=ops.ACT_RELU)
            tk = dict(pad=1, transposed=True, out_hw=(H, W))
            calls = {
                'fwd': (lambda: ops.conv2d(x, w, **kw), FWD[ops.conv2d_kernel_id(x, w, **kw)], x.numel() * 2 + dz.numel() * 2),
                'dgrad': (lambda: ops.conv2d(dz, w, **tk), FWD[ops.conv2d_kernel_id(dz, w, **tk)], x.numel() * 2 + dz.numel() * 2),
                'wgrad': (lambda: ops.conv2d_wgrad(x, dz, (co, 32, 3, 3), dw_out=sink, **kw),
                          WG[ops.conv2d_wgrad(x, dz, (co, 32, 3, 3), _query=True, **kw)], x.numel() * 2 + dz.numel() * 2),
            }
            for name, (fn, kern, nbytes) in calls.items():
                t = timed(fn, a.warmup, a.repeats)
                print(f'  {N} x {H} x {W}  Co {co:2d}  {name:5s}  {t[0]:8.3f} [{t[1]:.3f}, {t[2]:.3f}] ms  '
                      f'{nbytes / t[0] / 1e6:7.0f} GB/s  {kern}', flush=True)
            del w, dz, sink


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--repeats', type=int, default=20)
    p.add_argument('--classes', type=int, nargs='+', default=[11, 19, 32])
    p.add_argument('--child', action='store_true')
    p.add_argument('--out')
    a = p.parse_args()
    if a.child:
        return child(a)
    lines = [f'head_mc_bench: warmup {a.warmup}, repeats {a.repeats} (median [min, max] ms; GB/s = minimum traffic / median)']
    runs = [('LEDN_HEAD_MC=1', '1', a.classes), ('LEDN_HEAD_MC=0', '0', a.classes), ('two-class floor', '1', [2])]
    for title, knob, classes in runs:
        env = dict(os.environ, LEDN_EXPERIMENTAL='1', LEDN_HEAD_MC=knob)
        cmd = [sys.executable, osp.abspath(__file__), '--child', '--warmup', str(a.warmup), '--repeats', str(a.repeats),
               '--classes'] + [str(c) for c in classes]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f'{title}: child failed ({r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}')
        lines.append(title)
        lines += r.stdout.rstrip('\n').split('\n')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
