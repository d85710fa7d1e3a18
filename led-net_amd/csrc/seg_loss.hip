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
//
// FocalLoss (sigmoid form, focal_loss.py:13-68 on the flattening, one-hot and valid_mask of FocalLoss.forward's GPU
// branch, :241-284) rides the same kernels as a further KIND: per pixel and class, z = t ? -x : x, so that
// 1 - p_t = sigmoid(z) and -log p_t = softplus(z) = max(z, 0) + log1p(exp(-|z|)) (never log(sigmoid));
// sigmoid(z)^gamma = exp(gamma * log sigmoid(z)), log sigmoid(z) = min(z, 0) - log1p(exp(-|z|)): no pow, and gamma = 0
// gives exactly 1.  part: f0 = sum of the weighted elements; the finish divides by q.div (N*HW*C or 1).
//
// TverskyLoss (tversky_loss.py:13-123) needs three sums per (image, class), so its forward has kernels of its own
// (tv_*): a thread keeps 3 x CB accumulators in registers for CB classes per pass (CB = 2 for two classes, else 8: the
// pixel loop runs ceil(C / 8) times, re-forming the softmax, instead of 3 x 32 accumulators spilling to scratch).
// work layout (ledn_tversky_work_floats(N, C) = 5 N C + max(SL_GRID, N) (2 + 3 C)):
//   hdr[N][C][5] | cnt[N * G][2] | part[N * G][C][3]
//   hdr (written by the finish): TP, FP, FN, and the backward's dL/dp_i for t = 1 and for t = 0 (without dloss)
//   cnt (per workgroup, u32 bit patterns): #pixels with label != ignore_index, #of those whose argmax is the label
//   part (per workgroup): TP, FP, FN of each class
// Its backward is a KIND of the shared backward kernels: the 2 C coefficients of the image, times dloss, sit in LDS.
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

// Focal: L = log1p(exp(-|z|)), so that softplus(z) = max(z, 0) + L and log sigmoid(z) = min(z, 0) - L
__device__ __forceinline__ float sl_focal_alpha(const SlCfg& q, int c, bool t) {
    const float a = q.alpha_v ? q.alpha_v[c] : q.alpha;
    return (q.cw ? q.cw[c] : 1.f) * (t ? a : 1.f - a);
}
__device__ __forceinline__ float sl_focal_fwd(float x, bool t, int c, const SlCfg& q) {
    const float z = t ? -x : x;
    const float L = log1pf(__expf(-fabsf(z)));
    const float sp = fmaxf(z, 0.f) + L;
    const float mod = __expf(q.gamma * (fminf(z, 0.f) - L));
    return sl_focal_alpha(q, c, t) * mod * sp;
}
// d/dx of the above times k: d mod / dz = gamma mod (1 - s), d sp / dz = s, s = sigmoid(z), dz/dx = -+1
__device__ __forceinline__ float sl_focal_bwd(float x, bool t, int c, const SlCfg& q, float k) {
    const float z = t ? -x : x;
    const float e = __expf(-fabsf(z));
    const float L = log1pf(e);
    const float sp = fmaxf(z, 0.f) + L;
    const float mod = __expf(q.gamma * (fminf(z, 0.f) - L));
    const float r = 1.f / (1.f + e);
    const float s = z >= 0.f ? r : e * r, s1 = z >= 0.f ? e * r : r;          // sigmoid(z), 1 - sigmoid(z)
    const float g = k * sl_focal_alpha(q, c, t) * mod * (q.gamma * s1 * sp + s);
    return t ? -g : g;
}

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
    if constexpr (KIND == SL_FOCAL) {
        if (tg == q.ignore_index) return;
        for (int c = 0; c < C; ++c) a.f0 += sl_focal_fwd(lg[c], c == tg, c, q);
    } else if constexpr (KIND == SL_CE) {
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
// sigmoid or softmax Jacobian.  Focal: k_t = dloss * loss_weight / divisor.  Tversky: tv[2 c], tv[2 c + 1] = dL/dp_c of
// this image for t = 1 and t = 0 (dloss applied), on the pixels whose label is not the loss's ignore_index.
template <int KIND>
__device__ __forceinline__ void sl_pixel_bwd(const float* lg, int C, long long tg, const SlCfg& q, float k_t, float k_p,
                                             const float* tv, float* dl) {
    if constexpr (KIND == SL_FOCAL) {
        const float k = tg == q.ignore_index ? 0.f : k_t;
        for (int c = 0; c < C; ++c) dl[c] = sl_focal_bwd(lg[c], c == tg, c, q, k);
    } else if constexpr (KIND == SL_TVERSKY) {
        if (tg == q.ignore_class) {
            for (int c = 0; c < C; ++c) dl[c] = 0.f;
            return;
        }
        float mx = lg[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, lg[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf(lg[c] - mx);
        const float inv = 1.f / se;
        const int tc = tg < 0 ? 0 : (tg >= C ? C - 1 : (int)tg);
        float dot = 0.f;
        for (int c = 0; c < C; ++c) dot += tv[2 * c + (c == tc ? 0 : 1)] * (__expf(lg[c] - mx) * inv);
        for (int c = 0; c < C; ++c) dl[c] = __expf(lg[c] - mx) * inv * (tv[2 * c + (c == tc ? 0 : 1)] - dot);
    } else if constexpr (KIND == SL_DICE_SIGMOID) {
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
            if (kind == SL_CE || kind == SL_FOCAL) {
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
    } else if (kind == SL_FOCAL) {
        out[0] = q.loss_weight * (tot0 / q.div);
        out[2] = 0.f;
        out[3] = 0.f;
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
    } else if constexpr (KIND == SL_FOCAL) {
        k_t = g / q.div;
        k_p = 0.f;
    } else if constexpr (KIND == SL_TVERSKY) {
        k_t = k_p = 0.f;          // (its coefficients are per class: sl_tv_coef)
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

// Tversky: the 2 C backward coefficients of image n from hdr, times dloss, into LDS (C <= SL_TV_MAX_C)
__device__ __forceinline__ void sl_tv_coef(float* s_tv, const float* work, const float* dloss, int n, int C) {
    if ((int)threadIdx.x < 2 * C)
        s_tv[threadIdx.x] = dloss[0] * work[((long)n * C + (threadIdx.x >> 1)) * 5 + 3 + (threadIdx.x & 1)];
    __syncthreads();
}

template <int KIND>
__global__ void __launch_bounds__(256) sl_bwd_kernel(const float* logits, const long long* target, long HW, int C,
                                                     const SlCfg q, const float* work, const float* out,
                                                     const float* dloss, float* dlogits, int N) {
    const int n = blockIdx.y;
    float k_t, k_p;
    sl_bwd_coef<KIND>(q, work, out, dloss, n, N, k_t, k_p);
    const float* tv = nullptr;
    if constexpr (KIND == SL_TVERSKY) {
        __shared__ float s_tv[2 * SL_TV_MAX_C];
        sl_tv_coef(s_tv, work, dloss, n, C);
        tv = s_tv;
    }
    const float* lgn = logits + (long)n * HW * C;
    float* dn = dlogits + (long)n * HW * C;
    const long long* tn = target + (long)n * HW;
    const long stride = (long)gridDim.x * 256;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += stride) {
        if (C == 2) {
            const float2 v = *reinterpret_cast<const float2*>(lgn + p * 2);
            const float l2[2] = {v.x, v.y};
            float d2[2];
            sl_pixel_bwd<KIND>(l2, 2, tn[p], q, k_t, k_p, tv, d2);
            *reinterpret_cast<float2*>(dn + p * 2) = make_float2(d2[0], d2[1]);
        } else {
            sl_pixel_bwd<KIND>(lgn + p * C, C, tn[p], q, k_t, k_p, tv, dn + p * C);
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
    const float* tv = nullptr;
    if constexpr (KIND == SL_TVERSKY) {
        __shared__ float s_tv[4];
        sl_tv_coef(s_tv, work, dloss, n, 2);
        tv = s_tv;
    }
    const float* sn = src + (long)n * Hs * Ws * 2;
    const long long* tn = target + (long)n * H * W;
    for (int k = threadIdx.x; k < CHH * CHW; k += 512) {
        const int y = 2 * i0 - 1 + k / CHW, x = 2 * j0 - 1 + k % CHW;
        float2 g = make_float2(0.f, 0.f);
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const float2 v = sl_up(sn, Ws, lerp_coord(y, Hs, H), lerp_coord(x, Ws, W));
            const float l2[2] = {v.x, v.y};
            float d2[2];
            sl_pixel_bwd<KIND>(l2, 2, tn[(long)y * W + x], q, k_t, k_p, tv, d2);
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
// Tversky forward: classes c0 .. c0 + CB - 1 of one pixel into the thread's 3 x CB accumulators (CB a constant and the
// loops over it unrolled: registers, no scratch).  first: this pass also counts the accuracy.
// ---------------------------------------------------------------------------------------------------------------
constexpr int TV_HDR = 5;
long long tversky_work_floats(long long N, int C) {
    return TV_HDR * N * C + (N > SL_GRID ? N : (long long)SL_GRID) * (2 + 3LL * C);
}

template <int CB>
struct TvAcc {
    float tp[CB], fp[CB], fn[CB];
    unsigned u1, u2;
};

template <int CB>
__device__ __forceinline__ void tv_pixel_fwd(const float* lg, int C, int c0, long long tg, const SlCfg& q, TvAcc<CB>& a) {
    float mx = lg[0];
    int am = 0;
    for (int c = 1; c < C; ++c)
        if (lg[c] > mx) { mx = lg[c]; am = c; }
    if (c0 == 0 && tg != q.ignore_index) {
        ++a.u1;
        if (am == tg) ++a.u2;
    }
    if (tg == q.ignore_class) return;
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += __expf(lg[c] - mx);
    const float inv = 1.f / se;
    const int tc = tg < 0 ? 0 : (tg >= C ? C - 1 : (int)tg);
#pragma unroll
    for (int k = 0; k < CB; ++k) {
        const int c = c0 + k;
        if (c < C) {
            const float p = __expf(lg[c] - mx) * inv;
            a.tp[k] += c == tc ? p : 0.f;
            a.fn[k] += c == tc ? 1.f - p : 0.f;
            a.fp[k] += c == tc ? 0.f : p;
        }
    }
}

template <int CB>
__device__ __forceinline__ void tv_acc_clear(TvAcc<CB>& a) {
#pragma unroll
    for (int k = 0; k < CB; ++k) a.tp[k] = a.fp[k] = a.fn[k] = 0.f;
    a.u1 = a.u2 = 0u;
}

// the workgroup's sums of classes c0 .. -> part[slot][c][3] (wave sums, then the four waves in a fixed order); with
// c0 == 0 also its two counts -> cnt[slot][2].  Ends in a barrier: s_f may be reused at once.
template <int CB>
__device__ __forceinline__ void tv_block_write(const TvAcc<CB>& a, float (*s_f)[3 * CB], unsigned (*s_u)[2], int C, int c0,
                                               float* cnt, float* part) {
    const int wid = threadIdx.x >> 6;
    const bool l0 = lane_id() == 0;
#pragma unroll
    for (int k = 0; k < CB; ++k) {
        const float tp = wave_sum(a.tp[k]), fp = wave_sum(a.fp[k]), fn = wave_sum(a.fn[k]);
        if (l0) {
            s_f[wid][3 * k] = tp;
            s_f[wid][3 * k + 1] = fp;
            s_f[wid][3 * k + 2] = fn;
        }
    }
    if (c0 == 0) {
        const unsigned u1 = sl_wave_sum_u(a.u1), u2 = sl_wave_sum_u(a.u2);
        if (l0) { s_u[wid][0] = u1; s_u[wid][1] = u2; }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 3 * CB && c0 + t / 3 < C) part[3 * c0 + t] = (s_f[0][t] + s_f[1][t]) + (s_f[2][t] + s_f[3][t]);
    if (c0 == 0 && t < 2) cnt[t] = __uint_as_float(s_u[0][t] + s_u[1][t] + s_u[2][t] + s_u[3][t]);
    __syncthreads();
}

// generic: grid (G, N), one pixel per thread and step, ceil(C / CB) passes over the image's pixels
template <int CB>
__global__ void __launch_bounds__(256) tv_fwd_kernel(const float* logits, const long long* target, long HW, int C,
                                                     const SlCfg q, float* work, int N) {
    __shared__ float s_f[4][3 * CB];
    __shared__ unsigned s_u[4][2];
    const int n = blockIdx.y;
    const long slot = (long)n * gridDim.x + blockIdx.x, slots = (long)N * gridDim.x;
    float* cnt = work + (long)TV_HDR * N * C + 2 * slot;
    float* part = work + (long)TV_HDR * N * C + 2 * slots + slot * 3 * C;
    const float* lgn = logits + (long)n * HW * C;
    const long long* tn = target + (long)n * HW;
    const long stride = (long)gridDim.x * 256;
    for (int c0 = 0; c0 < C; c0 += CB) {
        TvAcc<CB> a;
        tv_acc_clear(a);
        for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += stride) {
            if constexpr (CB == 2) {          // (two classes)
                const float2 v = *reinterpret_cast<const float2*>(lgn + p * 2);
                const float l2[2] = {v.x, v.y};
                tv_pixel_fwd<CB>(l2, 2, 0, tn[p], q, a);
            } else {
                tv_pixel_fwd<CB>(lgn + p * C, C, c0, tn[p], q, a);
            }
        }
        tv_block_write<CB>(a, s_f, s_u, C, c0, cnt, part);
    }
}

// resize-folded (two classes): the walk of sl_up_fwd_kernel
__global__ void __launch_bounds__(256) tv_up_fwd_kernel(const float* src, int Hs, int Ws, const long long* target,
                                                        const SlCfg q, float* work, int N) {
    __shared__ float s_f[4][6];
    __shared__ unsigned s_u[4][2];
    const int n = blockIdx.y, H = 2 * Hs, W = 2 * Ws;
    const long slot = (long)n * gridDim.x + blockIdx.x, slots = (long)N * gridDim.x;
    const float* sn = src + (long)n * Hs * Ws * 2;
    const long long* tn = target + (long)n * H * W;
    const int nq = (W + 3) / 4;
    TvAcc<2> a;
    tv_acc_clear(a);
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
                    tv_pixel_fwd<2>(l2, 2, 0, tg[k], q, a);
                }
            }
        }
    }
    tv_block_write<2>(a, s_f, s_u, 2, 0, work + (long)TV_HDR * N * 2 + 2 * slot,
                      work + (long)TV_HDR * N * 2 + 2 * slots + slot * 6);
}

// finish: ONE workgroup.  Every (image, class, sum) series of G partials is added by one wave in a fixed order; then a
// thread per (image, class) forms the term and the backward's two coefficients, and the terms are added in a fixed order.
__global__ void __launch_bounds__(256) tv_finish_kernel(float* work, int N, int C, int G, const SlCfg q, float* out) {
    __shared__ float s_f[4];
    __shared__ unsigned s_u[4][2];
    const float* cnt = work + (long)TV_HDR * N * C;
    const float* part = cnt + 2L * N * G;
    const int wid = threadIdx.x >> 6, lane = lane_id();
    const long series = 3L * N * C;
    for (long e = wid; e < series; e += 4) {
        const long n = e / (3 * C);
        const int r = (int)(e % (3 * C));          // = 3 c + j
        float a = 0.f;
        for (int b = lane; b < G; b += 64) a += part[(n * G + b) * 3 * C + r];
        a = wave_sum(a);
        if (lane == 0) work[(n * C + r / 3) * TV_HDR + r % 3] = a;
    }
    unsigned u1 = 0u, u2 = 0u;          // < 2^31: the entry points require N*HW < 2^31
    for (long i = threadIdx.x; i < (long)N * G; i += 256) {
        u1 += __float_as_uint(cnt[2 * i]);
        u2 += __float_as_uint(cnt[2 * i + 1]);
    }
    u1 = sl_wave_sum_u(u1);
    u2 = sl_wave_sum_u(u2);
    if (lane == 0) { s_u[wid][0] = u1; s_u[wid][1] = u2; }
    __syncthreads();          // (the sums in hdr are the workgroup's own writes: visible after the barrier)
    float acc = 0.f;
    for (long e = threadIdx.x; e < (long)N * C; e += 256) {
        const int i = (int)(e % C);
        float* h = work + e * TV_HDR;
        const float TP = h[0], FP = h[1], FN = h[2];
        const float num = TP + q.eps, D = TP + q.alpha * FP + q.beta * FN + q.eps;
        const float w = i == q.ignore_class ? 0.f : (q.cw ? q.cw[i] : 1.f);
        acc += w * (1.f - num / D);
        const float K = w * q.loss_weight / ((float)C * (float)N), iD2 = 1.f / (D * D);
        h[3] = K * (-(D - num) - q.beta * num) * iD2;          // t = 1: d/dTP - d/dFN
        h[4] = K * (q.alpha * num) * iD2;                      // t = 0: d/dFP
    }
    acc = wave_sum(acc);
    if (lane == 0) s_f[wid] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned c1 = s_u[0][0] + s_u[1][0] + s_u[2][0] + s_u[3][0], c2 = s_u[0][1] + s_u[1][1] + s_u[2][1] + s_u[3][1];
    out[0] = q.loss_weight * (((s_f[0] + s_f[1]) + (s_f[2] + s_f[3])) / (float)N) / (float)C;
    out[1] = ((float)c2 + SL_F32_EPS) * (100.0f / ((float)c1 + SL_F32_EPS));
    out[2] = 0.f;
    out[3] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
#define SL_DISPATCH(kind, LAUNCH)                                \
    do {                                                         \
        if ((kind) == SL_CE) { LAUNCH(SL_CE); }                  \
        else if ((kind) == SL_DICE_SIGMOID) { LAUNCH(SL_DICE_SIGMOID); } \
        else if ((kind) == SL_FOCAL) { LAUNCH(SL_FOCAL); }       \
        else { LAUNCH(SL_DICE_SOFTMAX); }                        \
    } while (0)
// (Tversky shares the backward kernels only)
#define SL_DISPATCH_BWD(kind, LAUNCH)                            \
    do {                                                         \
        if ((kind) == SL_TVERSKY) { LAUNCH(SL_TVERSKY); }        \
        else SL_DISPATCH(kind, LAUNCH);                          \
    } while (0)

static bool sl_cfg_ok(int kind, const SlCfg& q) {
    if (kind < SL_CE || kind > SL_TVERSKY) return false;
    if (q.reduction != 0 && q.reduction != 1) return false;
    if (kind == SL_FOCAL) return q.gamma >= 0.f;
    return kind == SL_CE || q.eps >= 0.f;
}
// Focal: the divisor of the sum, from the host's sizes
static SlCfg sl_with_div(int kind, SlCfg q, long long elems) {
    q.div = kind == SL_FOCAL && q.reduction == 0 ? (float)elems : 1.f;
    return q;
}

int seg_loss_fwd_impl(int kind, const float* logits, const long long* target, int N, long long HW, int C, const SlCfg& q0,
                      float* work, float* out, hipStream_t s) {
    LEDN_REQUIRE(logits && target && work && out && N > 0 && N <= 65535 && HW > 0 && C > 1 && sl_cfg_ok(kind, q0));
    LEDN_REQUIRE((long long)N * HW < (1LL << 31) && (long long)N * HW * C < (1LL << 40));
    LEDN_REQUIRE(C != 2 || ((uintptr_t)logits & 7) == 0);
    const SlCfg q = sl_with_div(kind, q0, (long long)N * HW * C);
    if (kind == SL_TVERSKY) {
        LEDN_REQUIRE(C <= SL_TV_MAX_C);
        const int G = sl_grid(N, cdiv(HW, 256));
        const dim3 grid((unsigned)G, (unsigned)N);
        if (C == 2)
            LEDN_LAUNCH(tv_fwd_kernel<2>, grid, dim3(256), 0, s, logits, target, (long)HW, C, q, work, N);
        else
            LEDN_LAUNCH(tv_fwd_kernel<8>, grid, dim3(256), 0, s, logits, target, (long)HW, C, q, work, N);
        LEDN_LAUNCH(tv_finish_kernel, dim3(1), dim3(256), 0, s, work, N, C, G, q, out);
        return check_launch();
    }
    const int G = sl_grid(N, cdiv(HW, 256));
    const dim3 grid((unsigned)G, (unsigned)N);
#define SL_L(K) LEDN_LAUNCH(sl_fwd_kernel<K>, grid, dim3(256), 0, s, logits, target, (long)HW, C, q, work, N)
    SL_DISPATCH(kind, SL_L);
#undef SL_L
    LEDN_LAUNCH(sl_finish_kernel, dim3(1), dim3(256), 0, s, kind, work, N, G, (float)((long long)N * HW), q, out);
    return check_launch();
}

int seg_loss_bwd_impl(int kind, const float* logits, const long long* target, int N, long long HW, int C, const SlCfg& q0,
                      const float* work, const float* out, const float* dloss, float* dlogits, hipStream_t s) {
    LEDN_REQUIRE(logits && target && work && out && dloss && dlogits && N > 0 && N <= 65535 && HW > 0 && C > 1);
    LEDN_REQUIRE(sl_cfg_ok(kind, q0) && (long long)N * HW < (1LL << 31) && (long long)N * HW * C < (1LL << 40));
    LEDN_REQUIRE(kind != SL_TVERSKY || C <= SL_TV_MAX_C);
    const SlCfg q = sl_with_div(kind, q0, (long long)N * HW * C);
    LEDN_REQUIRE(C != 2 || (((uintptr_t)logits | (uintptr_t)dlogits) & 7) == 0);
    long g = 4 * SL_GRID / N;
    if (g < 1) g = 1;
    if (g > cdiv(HW, 256)) g = cdiv(HW, 256);
    const dim3 grid((unsigned)g, (unsigned)N);
#define SL_L(K) \
    LEDN_LAUNCH(sl_bwd_kernel<K>, grid, dim3(256), 0, s, logits, target, (long)HW, C, q, work, out, dloss, dlogits, N)
    SL_DISPATCH_BWD(kind, SL_L);
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
                         const SlCfg& q0, float* work, float* out, hipStream_t s) {
    LEDN_REQUIRE(sl_up_ok(src, target, N, Hs, Ws, H, W) && work && out && sl_cfg_ok(kind, q0));
    const SlCfg q = sl_with_div(kind, q0, (long long)N * H * W * 2);
    const int G = sl_grid(N, H);
    const dim3 grid((unsigned)G, (unsigned)N);
    if (kind == SL_TVERSKY) {
        LEDN_LAUNCH(tv_up_fwd_kernel, grid, dim3(256), 0, s, src, Hs, Ws, target, q, work, N);
        LEDN_LAUNCH(tv_finish_kernel, dim3(1), dim3(256), 0, s, work, N, 2, G, q, out);
        return check_launch();
    }
#define SL_L(K) LEDN_LAUNCH(sl_up_fwd_kernel<K>, grid, dim3(256), 0, s, src, Hs, Ws, target, q, work, N)
    SL_DISPATCH(kind, SL_L);
#undef SL_L
    LEDN_LAUNCH(sl_finish_kernel, dim3(1), dim3(256), 0, s, kind, work, N, G, (float)((long long)N * H * W), q, out);
    return check_launch();
}

int seg_loss_up_bwd_impl(int kind, const float* src, int N, int Hs, int Ws, int H, int W, const long long* target,
                         const SlCfg& q0, const float* work, const float* out, const float* dloss, float* dsrc,
                         hipStream_t s) {
    LEDN_REQUIRE(sl_up_ok(src, target, N, Hs, Ws, H, W) && work && out && dloss && dsrc && sl_cfg_ok(kind, q0));
    LEDN_REQUIRE(((uintptr_t)dsrc & 7) == 0);
    const SlCfg q = sl_with_div(kind, q0, (long long)N * H * W * 2);
    const long nb = (long)N * cdiv(Hs, 8) * cdiv(Ws, 64);
    LEDN_REQUIRE(nb < (1L << 31));
#define SL_L(K) \
    LEDN_LAUNCH(sl_up_bwd_kernel<K>, dim3((unsigned)nb), dim3(512), 0, s, src, N, Hs, Ws, target, q, work, out, dloss, dsrc)
    SL_DISPATCH_BWD(kind, SL_L);
#undef SL_L
    return check_launch();
}

}  // namespace ledn
