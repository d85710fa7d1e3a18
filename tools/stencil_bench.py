"""Micro-benchmark of the depthwise / SESP-pyramid kernels at the training step's shapes (bf16, batch 16): forward, data
gradient, weight gradient, each launch timed with HIP events (ops.start_timing) over rotating buffer sets whose total
exceeds the 256 MB Infinity Cache, so that every call streams from HBM as it does inside the step.
Pyramid cases carry a stride; the context-branch blocks' shapes (dilations [1,2,3,4], stride 1 and 2 at 1/8, 1/16 and 1/32
resolution) and the adjoint of their 3x3/s2 average-pool shortcut (with its addend) are included.  The dw cases time what
ops_train.dwconv2d_bwd launches: one fused call (dwconv2d_bwd) where dw3x3_bwd_tile_kernel applies, else data + weight.
    python tools/stencil_bench.py [--iters 24] [--only pyr|dw|avg] [--dw-bwd-wgs N]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=24)
    ap.add_argument('--only', default=None, help='run only the cases of this kind (pyr, dw, avg)')
    ap.add_argument('--dw-bwd-wgs', type=int, default=0, help='LEDN_OPT_DW_BWD_WORKGROUPS (0 = default)')
    args = ap.parse_args()
    import importlib
    importlib.import_module('led_net_amd')
    from led_net_amd import _lib, ops, ops_train as T
    if args.dw_bwd_wgs:
        _lib.get_lib().set_option(_lib.OPT_DW_BWD_WORKGROUPS, args.dw_bwd_wgs)
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(1)
    bf = torch.bfloat16

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(bf).to(dev)
    # (kind, N, H, W, channels, dilations, group size (dw) / stride (pyr))
    ctx = [1, 2, 3, 4]
    cases = [('pyr', 16, 128, 128, 16, [1, 1, 1, 1], 1), ('pyr', 16, 128, 128, 32, [1, 1, 1, 1], 1),
             ('pyr', 16, 128, 128, 32, ctx, 1), ('pyr', 16, 128, 128, 32, ctx, 2),
             ('pyr', 16, 64, 64, 64, ctx, 1), ('pyr', 16, 64, 64, 64, ctx, 2),
             ('pyr', 16, 32, 32, 128, ctx, 1), ('pyr', 16, 32, 32, 128, ctx, 2),
             ('dw', 16, 128, 128, 64, [2, 2, 2, 2], 16), ('dw', 16, 128, 128, 128, [2, 2, 2, 2], 32),
             ('dw', 16, 128, 128, 128, [2, 3, 4, 5], 32), ('dw', 16, 64, 64, 256, [2, 3, 4, 5], 64),
             # the context branch's other second-stage depthwise convs (LEDN_BENCH_VERBOSE table of the step): behind the
             # stride-2 pyramids at 1/16 and 1/32 resolution, and the 1/32 stride-1 blocks
             ('dw', 16, 64, 64, 128, [2, 3, 4, 5], 32), ('dw', 16, 32, 32, 256, [2, 3, 4, 5], 64),
             ('dw', 16, 32, 32, 512, [2, 3, 4, 5], 128),
             ('avg', 16, 128, 128, 128, None, 0), ('avg', 16, 64, 64, 256, None, 0), ('avg', 16, 32, 32, 512, None, 0)]
    for kind, N, H, W, n, dil, gs in cases:
        if args.only and kind != args.only:
            continue
        st = gs if kind == 'pyr' else 1
        Ho, Wo = (H - 1) // st + 1, (W - 1) // st + 1
        nset = max(2, int(400e6 // (N * H * W * (n * (10 if kind == 'pyr' else 4)))) + 1)
        sets = []
        for _ in range(nset):
            if kind == 'pyr':
                sets.append((rnd(N, H, W, n), rnd(N, Ho, Wo, 4 * n), (0.3 * torch.randn(4, 3, 3, n, generator=g)).to(dev)))
            elif kind == 'avg':
                sets.append((rnd(N, H, W, n), rnd(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, n), None))
            else:
                sets.append((rnd(N, H, W, n), rnd(N, H, W, n), (0.3 * torch.randn(3, 3, n, generator=g)).to(dev)))
        torch.cuda.synchronize()
        ops.start_timing()
        for it in range(args.iters):
            x, dy, w = sets[it % nset]
            if kind == 'pyr':
                ops.sesp_pyramid(x, w, dil, st)
                T.sesp_pyramid_bwd(x, dy, w, dil, st)
            elif kind == 'avg':
                T.avgpool3x3s2_bwd(dy, (H, W), add=x)
            else:
                ops.dwconv2d(x, w, dil=dil, group_size=gs)
                T.dwconv2d_bwd(x, dy, w, dil=dil, group_size=gs)
        torch.cuda.synchronize()
        rec = ops.stop_timing()
        agg = {}
        for r in rec:
            agg.setdefault(r['entry'], []).append(r['ms'] * 1e3)
        line = []
        for e, ts in agg.items():
            ts = sorted(ts[len(ts) // 4:])          # the first quarter warms up
            line.append(f'{e[5:]} {ts[len(ts) // 2]:6.1f}')
        print(f'{kind} {N}x{H}x{W} n{n} dil{dil}' + (f' s{st}' if kind == 'pyr' else '') + ': ' + ' | '.join(line) + ' us',
              flush=True)


if __name__ == '__main__':
    main()
