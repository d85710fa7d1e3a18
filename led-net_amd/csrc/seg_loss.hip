// seg_loss.hip -- CrossEntropyLoss (softmax form, mmseg/models/losses/cross_entropy_loss.py:12-78) and DiceLoss
// (dice_loss.py:11-91,141-188) for LEDHead.loss_by_feat, each as a generic family (NHWC logits [N,HW,C]) and a
// resize-folded family (src [N,Hs,Ws,2] -> the exact 2x bilinear resize applied on the fly, as ledn_ohem_ce_up_*).
//
// The choices measured for ohem_fused.hip are kept: persistent workgroups walk the rows, four consecutive pixels per
// thread (two 16-byte label loads, the eight source values of a row pair loaded once per quad), no same-address
// atomics.  What these losses do NOT need is everything per-pixel that OHEM stores: there is no selection, so the
// forward is ONE streaming pass that leaves five numbers per workgroup, a single-workgroup finish sums them in a fixed
// order (bit-reproducible, with or without LEDN_OPT_DETERMINISTIC), and the backward re-forms the probabilities from
// the logits.  The grid is (G, N): a workgroup belongs to one image, because Dice's sums are per image.
//
// work layout (floats): hdr[N][4] | part[N * G][5]            (ledn_seg_loss_work_floats(N): 4 N + 5 max(SL_GRID, N))
//   hdr  (Dice, written by the finish): a = sum p t, b = sum p^2 (naive: sum p), c = sum t, loss_n -- without eps
//   part (per workgroup): f0, f1, u0, u1, u2 (the three counts as u32 bit patterns: exact)
//        CE:   f0 = sum w[y] CE, f1 = sum w[y], u0 = #pixels in the loss
//        Dice: f0 = a, f1 = b, u0 = c
//        both: u1 = #pixels with label != ignore_index, u2 = #of those whose first-max argmax is the label (accuracy)
// out[4]: loss (loss_weight applied), accuracy in percent (the definition of ledn_ohem_ce_fwd's out[1]), CE: divisor and
// #pixels in the loss, Dice: 0, 0.
//
// CE: a pixel is in the loss when label != ignore_index and 0 <= label < C (a label outside that range would read past
// the logits; F.cross_entropy raises for it).  reduction 'mean' divides by (avg_factor + f32 eps) as
// losses/utils.py:75-79: avg_factor = sum of w[y] over the pixels in the loss with class weights, else their count
// (avg_non_ignore) or N*HW.  No pixel in the loss: loss 0, gradient 0.
// Dice: the one-hot target is clamp(label, 0, C) with row C dropped (dice_loss.py:24-29): a label >= C (255 = ignored)
// has target 0 in every class and still adds its p to the denominator, a negative label counts as class 0.
// ignore_class is the reference's class-CHANNEL drop (dice_loss.py:69-72).
#include "ledn_rt.h"

namespace ledn {

constexpr int SL_GRID = 1024;          // persistent workgroups of a forward pass over all images (4 per CU)
constexpr int SL_PART = 5;
constexpr float SL_F32_EPS = 1.1920929e-07f;

long long seg_loss_work_floats(long long N) { return 4 * N + SL_PART * (N > SL_GRID ? N : (long long)SL_GRID); }
static int sl_grid(int N, long units) {          // workgroups per image: N * G <= max(SL_GRID, N)
    long g = SL_GRID / N;
    if (g < 1) g = 1;
    return (int)(g < units ? g : units);
}

__device__ __forceinline__ unsigned sl_wave_sum_u(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

struct SlAcc {
    float f0, f1;
    unsigned u0, u1, u2;
};

// one pixel of the forward: lg[C] logits, tg its label
template <int KIND>
__device__ __forceinline__ void sl_pixel_fwd(const float* lg, int C, long long tg, const SlCfg& q, SlAcc& a) {
    float mx = lg[0];
    int am = 0;
    for (int c = 1; c < C; ++c)
        if (lg[c] > mx) { mx = lg[c]; am = c; }
    if (tg != q.ignore_index) {
        ++a.u1;
        if (am == tg) ++a.u2;
    }
    if constexpr (KIND == SL_CE) {
        if (tg == q.ignore_index || tg < 0 || tg >= C) return;
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf(lg[c] - mx);
        const float ce = __logf(se) - (lg[(int)tg] - mx);
        const float w = q.cw ? q.cw[(int)tg] : 1.f;
        a.f0 += w * ce;
        a.f1 += w;
        ++a.u0;
    } else {
        const int tc = tg < 0 ? 0 : (tg >= C ? -1 : (int)tg);
        float inv = 1.f;
        if constexpr (KIND == SL_DICE_SOFTMAX) {
            float se = 0.f;
            for (int c = 0; c < C; ++c) se += __expf(lg[c] - mx);
            inv = 1.f / se;
        }
        for (int c = 0; c < C; ++c) {
            if (c == q.ignore_class) continue;
            const float p = KIND == SL_DICE_SIGMOID ? 1.f / (1.f + __expf(-lg[c])) : __expf(lg[c] - mx) * inv;
            if (c == tc) {
                a.f0 += p;
                ++a.u0;
            }
            a.f1 += q.naive ? p : p * p;
        }
    }
}

// one pixel of the backward -> dl[C].  CE: k_t = dloss * loss_weight / divisor.  Dice: dL/dp_c = k_t t_c + k_p p_c
// (naive: k_t t_c + k_p) on the kept classes, both already scaled by loss_weight * dloss (/ N), pulled through the
// sigmoid or softmax Jacobian.
template <int KIND>
__device__ __forceinline__ void sl_pixel_bwd(const float* lg, int C, long long tg, const SlCfg& q, float k_t, float k_p,
                                             float* dl) {
    if constexpr (KIND == SL_DICE_SIGMOID) {
        const int tc = tg < 0 ? 0 : (tg >= C ? -1 : (int)tg);
        for (int c = 0; c < C; ++c) {
            const float p = 1.f / (1.f + __expf(-lg[c]));
            const float g = c == q.ignore_class ? 0.f : (c == tc ? k_t : 0.f) + (q.naive ? k_p : k_p * p);
            dl[c] = g * p * (1.f - p);
        }
    } else {
        const bool off = KIND == SL_CE && (tg == q.ignore_index || tg < 0 || tg >= C);
        if (off) {
            for (int c = 0; c < C; ++c) dl[c] = 0.f;
            return;
        }
        float mx = lg[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, lg[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf(lg[c] - mx);
        const float inv = 1.f / se;
        if constexpr (KIND == SL_CE) {
            const float cf = q.cw ? k_t * q.cw[(int)tg] : k_t;
            for (int c = 0; c < C; ++c) dl[c] = cf * (__expf(lg[c] - mx) * inv - (c == (int)tg ? 1.f : 0.f));
        } else {
            const int tc = tg < 0 ? 0 : (tg >= C ? -1 : (int)tg);
            float dot = 0.f;
            for (int c = 0; c < C; ++c) {
                const float p = __expf(lg[c] - mx) * inv;
                const float g = c == q.ignore_class ? 0.f : (c == tc ? k_t : 0.f) + (q.naive ? k_p : k_p * p);
                dot += g * p;
            }
            for (int c = 0; c < C; ++c) {
                const float p = __expf(lg[c] - mx) * inv;
                const float g = c == q.ignore_class ? 0.f : (c == tc ? k_t : 0.f) + (q.naive ? k_p : k_p * p);
                dl[c] = p * (g - dot);
            }
        }
    }
}

// the workgroup's five numbers -> part[0..4] (wave sums, then the four waves in a fixed order)
__device__ __forceinline__ void sl_block_write(const SlAcc& a, float (*s_f)[2], unsigned (*s_u)[3], float* part) {
    const float f0 = wave_sum(a.f0), f1 = wave_sum(a.f1);
    const unsigned u0 = sl_wave_sum_u(a.u0), u1 = sl_wave_sum_u(a.u1), u2 = sl_wave_sum_u(a.u2);
    const int wid = threadIdx.x >> 6;
    if (lane_id() == 0) {
        s_f[wid][0] = f0; s_f[wid][1] = f1;
        s_u[wid][0] = u0; s_u[wid][1] = u1; s_u[wid][2] = u2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[0] = (s_f[0][0] + s_f[1][0]) + (s_f[2][0] + s_f[3][0]);
        part[1] = (s_f[0][1] + s_f[1][1]) + (s_f[2][1] + s_f[3][1]);
#pragma unroll
        for (int i = 0; i < 3; ++i) part[2 + i] = __uint_as_float(s_u[0][i] + s_u[1][i] + s_u[2][i] + s_u[3][i]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// generic forward: grid (G, N), one pixel per thread and step
// ---------------------------------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(256) sl_fwd_kernel(const float* logits, const long long* target, long HW, int C,
                                                     const SlCfg q, float* work, int N) {
    __shared__ float s_f[4][2];
    __shared__ unsigned s_u[4][3];
    const int n = blockIdx.y;
    const float* lgn = logits + (long)n * HW * C;
    const long long* tn = target + (long)n * HW;
    SlAcc a = {0.f, 0.f, 0u, 0u, 0u};
    const long stride = (long)gridDim.x * 256;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += stride) {
        if (C == 2) {
            const float2 v = *reinterpret_cast<const float2*>(lgn + p * 2);
            const float l2[2] = {v.x, v.y};
            sl_pixel_fwd<KIND>(l2, 2, tn[p], q, a);
        } else {
            sl_pixel_fwd<KIND>(lgn + p * C, C, tn[p], q, a);
        }
    }
    sl_block_write(a, s_f, s_u, work + 4L * N + ((long)n * gridDim.x + blockIdx.x) * SL_PART);
}

// ---------------------------------------------------------------------------------------------------------------
// resize-folded forward (exact 2x, two classes): grid (G, N), a workgroup walks rows y = blockIdx.x, + G, ... of its
// image, a thread takes quads of four consecutive pixels.  W = 2 Ws is even, so a quad is whole or (the last one of a
// W % 4 == 2 row) holds two pixels: the same loop handles it with the second label load and two pixels switched off.
// Returns the number of pixels of the quad.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float2 sl_mix(float wy0, float wy1, float wx0, float wx1, float2 v00, float2 v01, float2 v10,
                                         float2 v11) {
    float2 r;
    r.x = wy0 * (wx0 * v00.x + wx1 * v01.x) + wy1 * (wx0 * v10.x + wx1 * v11.x);
    r.y = wy0 * (wx0 * v00.y + wx1 * v01.y) + wy1 * (wx0 * v10.y + wx1 * v11.y);
    return r;
}
__device__ __forceinline__ float2 sl_up(const float* sn, int Ws, const Lerp& ly, const Lerp& lx) {
    const float2 v00 = *reinterpret_cast<const float2*>(sn + ((long)ly.i0 * Ws + lx.i0) * 2);
    const float2 v01 = *reinterpret_cast<const float2*>(sn + ((long)ly.i0 * Ws + lx.i1) * 2);
    const float2 v10 = *reinterpret_cast<const float2*>(sn + ((long)ly.i1 * Ws + lx.i0) * 2);
    const float2 v11 = *reinterpret_cast<const float2*>(sn + ((long)ly.i1 * Ws + lx.i1) * 2);
    return sl_mix(ly.w0, ly.w1, lx.w0, lx.w1, v00, v01, v10, v11);
}
__device__ __forceinline__ int sl_quad(const float* sn, const long long* trow, int Ws, int W, const Lerp& ly, int qx,
                                       float2* lg, long long* tg) {
    const int x0 = 4 * qx;
    const int cnt = W - x0 < 4 ? W - x0 : 4;
    {
        const uint4 a = *reinterpret_cast<const uint4*>(trow + x0);          // 2 x int64 per 16-byte load
        tg[0] = (long long)(((unsigned long long)a.y << 32) | a.x);
        tg[1] = (long long)(((unsigned long long)a.w << 32) | a.z);
        tg[2] = tg[3] = 0;
        if (cnt == 4) {
            const uint4 b = *reinterpret_cast<const uint4*>(trow + x0 + 2);
            tg[2] = (long long)(((unsigned long long)b.y << 32) | b.x);
            tg[3] = (long long)(((unsigned long long)b.w << 32) | b.z);
        }
    }
    // a whole quad away from the left / right border: pixels 4q .. 4q+3 interpolate source columns 2q-1 .. 2q+2 with
    // the weights (.25 .75) (.75 .25) (.25 .75) (.75 .25) -- what lerp_coord returns there (scale 0.5: every coordinate
    // is an exact multiple of 0.25)
    if (cnt == 4 && qx >= 1 && 2 * qx + 2 <= Ws - 1) {
        float2 c[2][4];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const float* rowp = sn + ((long)(rr ? ly.i1 : ly.i0) * Ws + 2 * qx - 1) * 2;
#pragma unroll
            for (int i = 0; i < 4; ++i) c[rr][i] = *reinterpret_cast<const float2*>(rowp + 2 * i);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            constexpr int ci[4] = {0, 1, 1, 2};
            const float wx1 = (k & 1) ? 0.25f : 0.75f, wx0 = 1.f - wx1;
            lg[k] = sl_mix(ly.w0, ly.w1, wx0, wx1, c[0][ci[k]], c[0][ci[k] + 1], c[1][ci[k]], c[1][ci[k] + 1]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lg[k] = make_float2(0.f, 0.f);
            if (k < cnt) lg[k] = sl_up(sn, Ws, ly, lerp_coord(x0 + k, Ws, W));
        }
    }
    return cnt;
}

template <int KIND>
__global__ void __launch_bounds__(256) sl_up_fwd_kernel(const float* src, int Hs, int Ws, const long long* target,
                                                        const SlCfg q, float* work, int N) {
    __shared__ float s_f[4][2];
    __shared__ unsigned s_u[4][3];
    const int n = blockIdx.y, H = 2 * Hs, W = 2 * Ws;
    const float* sn = src + (long)n * Hs * Ws * 2;
    const long long* tn = target + (long)n * H * W;
    const int nq = (W + 3) / 4;
    SlAcc a = {0.f, 0.f, 0u, 0u, 0u};
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const Lerp ly = lerp_coord(y, Hs, H);
        for (int qx = threadIdx.x; qx < nq; qx += 256) {
            float2 lg[4];
            long long tg[4];
            const int cnt = sl_quad(sn, tn + (long)y * W, Ws, W, ly, qx, lg, tg);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < cnt) {
                    const float l2[2] = {lg[k].x, lg[k].y};
                    sl_pixel_fwd<KIND>(l2, 2, tg[k], q, a);
                }
            }
        }
    }
    sl_block_write(a, s_f, s_u, work + 4L * N + ((long)n * gridDim.x + blockIdx.x) * SL_PART);
}

// ---------------------------------------------------------------------------------------------------------------
// finish: ONE workgroup sums the G partials of every image in a fixed order, forms the divisor / the per-image Dice
// terms on the device and writes out[4] (and hdr for Dice's backward)
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sl_finish_kernel(int kind, float* work, int N, int G, float npix, const SlCfg q,
                                                        float* out) {
    __shared__ float s_f[4][2];
    __shared__ unsigned s_u[4][3];
    const float* part = work + 4L * N;
    float tot0 = 0.f, tot1 = 0.f, loss_sum = 0.f;          // (thread 0)
    unsigned cnt0 = 0u, cnt1 = 0u, cnt2 = 0u;               // < 2^31: the entry points require N*HW < 2^31
    for (int n = 0; n < N; ++n) {
        SlAcc a = {0.f, 0.f, 0u, 0u, 0u};
        for (int b = threadIdx.x; b < G; b += 256) {
            const float* p = part + ((long)n * G + b) * SL_PART;
            a.f0 += p[0];
            a.f1 += p[1];
            a.u0 += __float_as_uint(p[2]);
            a.u1 += __float_as_uint(p[3]);
            a.u2 += __float_as_uint(p[4]);
        }
        const float f0 = wave_sum(a.f0), f1 = wave_sum(a.f1);
        const unsigned u0 = sl_wave_sum_u(a.u0), u1 = sl_wave_sum_u(a.u1), u2 = sl_wave_sum_u(a.u2);
        const int wid = threadIdx.x >> 6;
        if (lane_id() == 0) {
            s_f[wid][0] = f0; s_f[wid][1] = f1;
            s_u[wid][0] = u0; s_u[wid][1] = u1; s_u[wid][2] = u2;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const float F0 = (s_f[0][0] + s_f[1][0]) + (s_f[2][0] + s_f[3][0]);
            const float F1 = (s_f[0][1] + s_f[1][1]) + (s_f[2][1] + s_f[3][1]);
            const unsigned U0 = s_u[0][0] + s_u[1][0] + s_u[2][0] + s_u[3][0];
            cnt1 += s_u[0][1] + s_u[1][1] + s_u[2][1] + s_u[3][1];
            cnt2 += s_u[0][2] + s_u[1][2] + s_u[2][2] + s_u[3][2];
            if (kind == SL_CE) {
                tot0 += F0;
                tot1 += F1;
                cnt0 += U0;
            } else {
                const float a_ = F0, c_ = (float)U0;
                float ln;
                if (q.naive) {
                    ln = 1.f - (2.f * a_ + q.eps) / (F1 + c_ + q.eps);
                } else {
                    const float b = F1 + q.eps, c = c_ + q.eps;
                    ln = 1.f - (2.f * a_) / (b + c);
                }
                work[4 * n + 0] = a_;
                work[4 * n + 1] = F1;
                work[4 * n + 2] = c_;
                work[4 * n + 3] = ln;
                loss_sum += ln;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    out[1] = ((float)cnt2 + SL_F32_EPS) * (100.0f / ((float)cnt1 + SL_F32_EPS));
    if (kind == SL_CE) {
        float div = 1.f;
        if (q.reduction == 0) div = (q.cw ? tot1 : (q.avg_non_ignore ? (float)cnt0 : npix)) + SL_F32_EPS;
        out[0] = cnt0 == 0u ? 0.f : q.loss_weight * (tot0 / div);
        out[2] = div;
        out[3] = (float)cnt0;
    } else {
        out[0] = q.loss_weight * (q.reduction == 0 ? loss_sum / (float)N : loss_sum);
        out[2] = 0.f;
        out[3] = 0.f;
    }
}

// the backward's two coefficients of image n (see sl_pixel_bwd)
template <int KIND>
__device__ __forceinline__ void sl_bwd_coef(const SlCfg& q, const float* work, const float* out, const float* dloss, int n,
                                            int N, float& k_t, float& k_p) {
    const float g = dloss[0] * q.loss_weight;
    if constexpr (KIND == SL_CE) {
        k_t = out[3] > 0.f ? g / out[2] : 0.f;
        k_p = 0.f;
    } else {
        const float sc = q.reduction == 0 ? g / (float)N : g;
        const float a = work[4 * n], b = work[4 * n + 1], c = work[4 * n + 2];
        if (q.naive) {
            const float D = b + c + q.eps;
            k_t = sc * (-2.f / D);
            k_p = sc * ((2.f * a + q.eps) / (D * D));
        } else {
            const float D = (b + q.eps) + (c + q.eps);
            k_t = sc * (-2.f / D);
            k_p = sc * (4.f * a / (D * D));
        }
    }
}

template <int KIND>
__global__ void __launch_bounds__(256) sl_bwd_kernel(const float* logits, const long long* target, long HW, int C,
                                                     const SlCfg q, const float* work, const float* out,
                                                     const float* dloss, float* dlogits, int N) {
    const int n = blockIdx.y;
    float k_t, k_p;
    sl_bwd_coef<KIND>(q, work, out, dloss, n, N, k_t, k_p);
    const float* lgn = logits + (long)n * HW * C;
    float* dn = dlogits + (long)n * HW * C;
    const long long* tn = target + (long)n * HW;
    const long stride = (long)gridDim.x * 256;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += stride) {
        if (C == 2) {
            const float2 v = *reinterpret_cast<const float2*>(lgn + p * 2);
            const float l2[2] = {v.x, v.y};
            float d2[2];
            sl_pixel_bwd<KIND>(l2, 2, tn[p], q, k_t, k_p, d2);
            *reinterpret_cast<float2*>(dn + p * 2) = make_float2(d2[0], d2[1]);
        } else {
            sl_pixel_bwd<KIND>(lgn + p * C, C, tn[p], q, k_t, k_p, dn + p * C);
        }
    }
}

// resize-folded backward (as ohem2_bwd_up2_kernel): a workgroup owns 8 x 64 source pixels; the logit gradients of its
// 18 x 130 children are formed once in LDS (the logits re-interpolated from src), then every source pixel gathers its
// 4 x 4 children with the interpolation weights -- the adjoint of the resize without the full-resolution gradient.
template <int KIND>
__global__ void __launch_bounds__(512) sl_up_bwd_kernel(const float* src, int N, int Hs, int Ws, const long long* target,
                                                        const SlCfg q, const float* work, const float* out,
                                                        const float* dloss, float* dsrc) {
    constexpr int TH = 8, TW = 64, CHH = 2 * TH + 2, CHW = 2 * TW + 2;
    __shared__ float2 s_g[CHH * CHW];
    const int H = 2 * Hs, W = 2 * Ws;
    const int tw = (Ws + TW - 1) / TW, th = (Hs + TH - 1) / TH;
    const int bj = blockIdx.x % tw, bi = (blockIdx.x / tw) % th, n = blockIdx.x / (tw * th);
    const int i0 = bi * TH, j0 = bj * TW;
    float k_t, k_p;
    sl_bwd_coef<KIND>(q, work, out, dloss, n, N, k_t, k_p);
    const float* sn = src + (long)n * Hs * Ws * 2;
    const long long* tn = target + (long)n * H * W;
    for (int k = threadIdx.x; k < CHH * CHW; k += 512) {
        const int y = 2 * i0 - 1 + k / CHW, x = 2 * j0 - 1 + k % CHW;
        float2 g = make_float2(0.f, 0.f);
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const float2 v = sl_up(sn, Ws, lerp_coord(y, Hs, H), lerp_coord(x, Ws, W));
            const float l2[2] = {v.x, v.y};
            float d2[2];
            sl_pixel_bwd<KIND>(l2, 2, tn[(long)y * W + x], q, k_t, k_p, d2);
            g = make_float2(d2[0], d2[1]);
        }
        s_g[k] = g;
    }
    __syncthreads();
    const int a = threadIdx.x / TW, b = threadIdx.x % TW, i = i0 + a, j = j0 + b;
    if (i >= Hs || j >= Ws) return;
    float wys[4], wxs[4];         // the interpolation weight of child (dy, dx) onto this source pixel = wys[dy] * wxs[dx]
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int y = 2 * i - 1 + d, x = 2 * j - 1 + d;
        wys[d] = wxs[d] = 0.f;
        if (y >= 0 && y < H) {
            const Lerp ly = lerp_coord(y, Hs, H);
            wys[d] = (ly.i0 == i ? ly.w0 : 0.f) + (ly.i1 == i ? ly.w1 : 0.f);
        }
        if (x >= 0 && x < W) {
            const Lerp lx = lerp_coord(x, Ws, W);
            wxs[d] = (lx.i0 == j ? lx.w0 : 0.f) + (lx.i1 == j ? lx.w1 : 0.f);
        }
    }
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) {
            const float wgt = wys[dy] * wxs[dx];
            const float2 g = s_g[(2 * a + dy) * CHW + 2 * b + dx];
            acc.x += wgt * g.x;
            acc.y += wgt * g.y;
        }
    }
    *reinterpret_cast<float2*>(dsrc + (((long)n * Hs + i) * Ws + j) * 2) = acc;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
#define SL_DISPATCH(kind, LAUNCH)                                \
    do {                                                         \
        if ((kind) == SL_CE) { LAUNCH(SL_CE); }                  \
        else if ((kind) == SL_DICE_SIGMOID) { LAUNCH(SL_DICE_SIGMOID); } \
        else { LAUNCH(SL_DICE_SOFTMAX); }                        \
    } while (0)

static bool sl_cfg_ok(int kind, const SlCfg& q) {
    if (kind < SL_CE || kind > SL_DICE_SOFTMAX) return false;
    if (q.reduction != 0 && q.reduction != 1) return false;
    return kind == SL_CE || q.eps >= 0.f;
}

int seg_loss_fwd_impl(int kind, const float* logits, const long long* target, int N, long long HW, int C, const SlCfg& q,
                      float* work, float* out, hipStream_t s) {
    LEDN_REQUIRE(logits && target && work && out && N > 0 && N <= 65535 && HW > 0 && C > 1 && sl_cfg_ok(kind, q));
    LEDN_REQUIRE((long long)N * HW < (1LL << 31) && (long long)N * HW * C < (1LL << 40));
    LEDN_REQUIRE(C != 2 || ((uintptr_t)logits & 7) == 0);
    const int G = sl_grid(N, cdiv(HW, 256));
    const dim3 grid((unsigned)G, (unsigned)N);
#define SL_L(K) LEDN_LAUNCH(sl_fwd_kernel<K>, grid, dim3(256), 0, s, logits, target, (long)HW, C, q, work, N)
    SL_DISPATCH(kind, SL_L);
#undef SL_L
    LEDN_LAUNCH(sl_finish_kernel, dim3(1), dim3(256), 0, s, kind, work, N, G, (float)((long long)N * HW), q, out);
    return check_launch();
}

int seg_loss_bwd_impl(int kind, const float* logits, const long long* target, int N, long long HW, int C, const SlCfg& q,
                      const float* work, const float* out, const float* dloss, float* dlogits, hipStream_t s) {
    LEDN_REQUIRE(logits && target && work && out && dloss && dlogits && N > 0 && N <= 65535 && HW > 0 && C > 1);
    LEDN_REQUIRE(sl_cfg_ok(kind, q) && (long long)N * HW < (1LL << 31) && (long long)N * HW * C < (1LL << 40));
    LEDN_REQUIRE(C != 2 || (((uintptr_t)logits | (uintptr_t)dlogits) & 7) == 0);
    long g = 4 * SL_GRID / N;
    if (g < 1) g = 1;
    if (g > cdiv(HW, 256)) g = cdiv(HW, 256);
    const dim3 grid((unsigned)g, (unsigned)N);
#define SL_L(K) \
    LEDN_LAUNCH(sl_bwd_kernel<K>, grid, dim3(256), 0, s, logits, target, (long)HW, C, q, work, out, dloss, dlogits, N)
    SL_DISPATCH(kind, SL_L);
#undef SL_L
    return check_launch();
}

static bool sl_up_ok(const float* src, const long long* target, int N, int Hs, int Ws, int H, int W) {
    if (!src || !target || N <= 0 || N > 65535 || Hs <= 0 || Ws <= 0) return false;
    if (H != 2 * Hs || W != 2 * Ws) return false;                                    // the exact 2x resize only
    if (((uintptr_t)src & 7) != 0 || ((uintptr_t)target & 15) != 0) return false;    // float2 / 2 x int64 accesses
    return (long long)N * H * W < (1LL << 31);
}

int seg_loss_up_fwd_impl(int kind, const float* src, int N, int Hs, int Ws, int H, int W, const long long* target,
                         const SlCfg& q, float* work, float* out, hipStream_t s) {
    LEDN_REQUIRE(sl_up_ok(src, target, N, Hs, Ws, H, W) && work && out && sl_cfg_ok(kind, q));
    const int G = sl_grid(N, H);
    const dim3 grid((unsigned)G, (unsigned)N);
#define SL_L(K) LEDN_LAUNCH(sl_up_fwd_kernel<K>, grid, dim3(256), 0, s, src, Hs, Ws, target, q, work, N)
    SL_DISPATCH(kind, SL_L);
#undef SL_L
    LEDN_LAUNCH(sl_finish_kernel, dim3(1), dim3(256), 0, s, kind, work, N, G, (float)((long long)N * H * W), q, out);
    return check_launch();
}

int seg_loss_up_bwd_impl(int kind, const float* src, int N, int Hs, int Ws, int H, int W, const long long* target,
                         const SlCfg& q, const float* work, const float* out, const float* dloss, float* dsrc,
                         hipStream_t s) {
    LEDN_REQUIRE(sl_up_ok(src, target, N, Hs, Ws, H, W) && work && out && dloss && dsrc && sl_cfg_ok(kind, q));
    LEDN_REQUIRE(((uintptr_t)dsrc & 7) == 0);
    const long nb = (long)N * cdiv(Hs, 8) * cdiv(Ws, 64);
    LEDN_REQUIRE(nb < (1L << 31));
#define SL_L(K) \
    LEDN_LAUNCH(sl_up_bwd_kernel<K>, dim3((unsigned)nb), dim3(512), 0, s, src, N, Hs, Ws, target, q, work, out, dloss, dsrc)
    SL_DISPATCH(kind, SL_L);
#undef SL_L
    return check_launch();
}

}  // namespace ledn
