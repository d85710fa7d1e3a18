// tta_merge.hip -- merging of inference results at the ORIGINAL resolution: one test-time-augmentation view into the
// image's accumulator (un-pad, un-flip, bilinear resize, softmax, add; mean + argmax on the last view) and the
// sliding-window canvas (window += crop; divide by the window count + argmax).  HBM-bound on the planar f32
// accumulator [C][Ho][Wo]: lanes run along x, a lane owns PX consecutive x of every channel plane (PX = 4: one 16-byte
// access per plane), the view's logits are gathered through L2.  One writer per element per launch, no atomics.
#include "ledn_rt.h"

namespace ledn {

// PX consecutive f32 of one plane row / PX mask bytes
template <int PX> __device__ __forceinline__ void ldpx(const float* p, float* o) { ldv<PX>(p, o); }
template <int PX> __device__ __forceinline__ void stpx(float* p, const float* v) { stv<PX>(p, v); }
template <int PX> __device__ __forceinline__ void st_mask(unsigned char* p, const int* b) {
    if constexpr (PX == 4) {
        *reinterpret_cast<unsigned*>(p) = (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j) p[j] = (unsigned char)b[j];
    }
}

// logits of source pixel (y, x): NHWC [Hs][Ws][C] (one contiguous run) or planar [C][Hs][Ws]
template <int C, bool PLANAR> __device__ __forceinline__ void ld_src(const float* s, int y, int x, int Hs, int Ws, float* o) {
    if constexpr (PLANAR) {
        const long plane = (long)Hs * Ws, off = (long)y * Ws + x;
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = s[c * plane + off];
    } else {
        ldv<C>(s + ((long)y * Ws + x) * C, o);
    }
}

template <int C, int PX, bool PLANAR>
__global__ void __launch_bounds__(256) tta_accumulate_kernel(ledn_tta_desc d) {
    const unsigned wq = (unsigned)(d.Wo / PX);
    const unsigned total = (unsigned)d.Ho * wq;
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const unsigned ho = idx / wq;
    const int wo0 = (int)(idx - ho * wq) * PX;
    const long plane = (long)d.Ho * d.Wo, off = (long)ho * d.Wo + wo0;
    Lerp ly = lerp_coord((int)ho, d.hv, d.Ho);
    if (d.flip == LEDN_FLIP_VERTICAL) {          // row i of the un-flipped view is row hv-1-i of the source
        ly.i0 = d.hv - 1 - ly.i0;
        ly.i1 = d.hv - 1 - ly.i1;
    }
    float v[PX][C];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        Lerp lx = lerp_coord(wo0 + j, d.wv, d.Wo);
        if (d.flip == LEDN_FLIP_HORIZONTAL) {
            lx.i0 = d.wv - 1 - lx.i0;
            lx.i1 = d.wv - 1 - lx.i1;
        }
        float v00[C], v01[C], v10[C], v11[C];
        ld_src<C, PLANAR>(d.src, ly.i0, lx.i0, d.Hs, d.Ws, v00);
        ld_src<C, PLANAR>(d.src, ly.i0, lx.i1, d.Hs, d.Ws, v01);
        ld_src<C, PLANAR>(d.src, ly.i1, lx.i0, d.Hs, d.Ws, v10);
        ld_src<C, PLANAR>(d.src, ly.i1, lx.i1, d.Hs, d.Ws, v11);
        float m = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {      // the arithmetic of bilinear_nchw_kernel
            v[j][c] = lerp_blend(ly, lx, v00[c], v01[c], v10[c], v11[c]);
            m = (c == 0 || v[j][c] > m) ? v[j][c] : m;
        }
        if (d.mode == LEDN_TTA_SOFTMAX) {
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                v[j][c] = expf(v[j][c] - m);
                sum += v[j][c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) v[j][c] = v[j][c] / sum;
        }
    }
    const float kf = (float)d.K;
    int best[PX] = {};
    float bv[PX] = {};
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float a[PX];
        if (!d.first) {
            ldpx<PX>(d.acc + c * plane + off, a);
#pragma unroll
            for (int j = 0; j < PX; ++j) a[j] += v[j][c];
        } else {
#pragma unroll
            for (int j = 0; j < PX; ++j) a[j] = 0.f + v[j][c];
        }
        if (d.last) {
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                a[j] = a[j] / kf;
                if (c == 0 || a[j] > bv[j]) {
                    bv[j] = a[j];
                    best[j] = c;
                }
            }
        }
        stpx<PX>(d.acc + c * plane + off, a);
    }
    if (d.last && d.mask) st_mask<PX>(d.mask + off, best);
}

template <int C, int PX>
static int tta_launch(const ledn_tta_desc& d, hipStream_t s) {
    const dim3 grid((unsigned)cdiv((long)d.Ho * (d.Wo / PX), 256));
    if (d.src_planar) LEDN_LAUNCH((tta_accumulate_kernel<C, PX, true>), grid, dim3(256), 0, s, d);
    else LEDN_LAUNCH((tta_accumulate_kernel<C, PX, false>), grid, dim3(256), 0, s, d);
    return check_launch();
}

static bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int tta_accumulate_impl(const ledn_tta_desc& d, hipStream_t s) {
    LEDN_REQUIRE(d.src && d.acc);
    LEDN_REQUIRE(d.Hs > 0 && d.Ws > 0 && d.Ho > 0 && d.Wo > 0 && d.K > 0);
    LEDN_REQUIRE(d.hv > 0 && d.hv <= d.Hs && d.wv > 0 && d.wv <= d.Ws);
    LEDN_REQUIRE((long)d.Ho * d.Wo < 0x7fffffffL && (long)d.Hs * d.Ws * d.C < 0x7fffffffL);
    LEDN_REQUIRE(d.flip == LEDN_FLIP_NONE || d.flip == LEDN_FLIP_HORIZONTAL || d.flip == LEDN_FLIP_VERTICAL);
    LEDN_REQUIRE(d.mode == LEDN_TTA_SOFTMAX || d.mode == LEDN_TTA_RAW);
    LEDN_REQUIRE(aligned(d.src, 4) && aligned(d.acc, 4));
    if (!d.src_planar) LEDN_REQUIRE((d.C != 2 || aligned(d.src, 8)) && (d.C % 4 != 0 || aligned(d.src, 16)));
    // 16 B per lane on the accumulator planes (4 mask bytes per lane) when rows and planes keep the alignment
    const bool v4 = d.Wo % 4 == 0 && aligned(d.acc, 16) && (!d.mask || aligned(d.mask, 4));
#define LEDN_TTA(C) return v4 ? tta_launch<C, 4>(d, s) : tta_launch<C, 1>(d, s)
    switch (d.C) {
        case 2: LEDN_TTA(2);
        case 3: LEDN_TTA(3);
        case 4: LEDN_TTA(4);
        case 5: LEDN_TTA(5);
        case 8: LEDN_TTA(8);
        case 19: LEDN_TTA(19);
        default: return LEDN_EINVAL;
    }
#undef LEDN_TTA
}

// ---- sliding windows: canvas[n, c, y1 + y, x1 + x] += crop[n, y, x, c]  (crop NHWC or planar) -------------------------
template <int C, int PX, bool PLANAR>
__global__ void __launch_bounds__(256) slide_accumulate_kernel(float* canvas, const float* crop, int N, int H, int W,
                                                               int y1, int x1, int hc, int wc) {
    const unsigned wq = (unsigned)(wc / PX);
    const unsigned total = (unsigned)N * hc * wq;
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const unsigned row = idx / wq, n = row / (unsigned)hc;
    const int x = (int)(idx - row * wq) * PX, y = (int)(row - n * (unsigned)hc);
    const long plane = (long)H * W;
    float* cv = canvas + (long)n * C * plane + (long)(y1 + y) * W + x1 + x;
    float v[PX][C];
    if constexpr (PLANAR) {
        const float* cp = crop + (long)n * C * hc * wc + (long)y * wc + x;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float t[PX];
            ldpx<PX>(cp + (long)c * hc * wc, t);
#pragma unroll
            for (int j = 0; j < PX; ++j) v[j][c] = t[j];
        }
    } else {
        const float* cp = crop + (((long)n * hc + y) * wc + x) * C;
#pragma unroll
        for (int j = 0; j < PX; ++j) ldv<C>(cp + j * C, v[j]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float a[PX];
        ldpx<PX>(cv + c * plane, a);
#pragma unroll
        for (int j = 0; j < PX; ++j) a[j] += v[j][c];
        stpx<PX>(cv + c * plane, a);
    }
}

int slide_accumulate_impl(float* canvas, const float* crop, int N, int C, int H, int W, int y1, int x1, int hc, int wc,
                          int crop_planar, hipStream_t s) {
    LEDN_REQUIRE(canvas && crop && N > 0 && H > 0 && W > 0 && hc > 0 && wc > 0);
    LEDN_REQUIRE(y1 >= 0 && x1 >= 0 && (long)y1 + hc <= H && (long)x1 + wc <= W);
    LEDN_REQUIRE((long)N * C * H * W < 0x7fffffffL * 4L && (long)N * hc * wc < 0x7fffffffL);
    LEDN_REQUIRE(aligned(canvas, 4) && aligned(crop, 4));
    if (!crop_planar) LEDN_REQUIRE((C != 2 || aligned(crop, 8)) && (C % 4 != 0 || aligned(crop, 16)));
    const bool v4 = W % 4 == 0 && x1 % 4 == 0 && wc % 4 == 0 && aligned(canvas, 16) && (!crop_planar || aligned(crop, 16));
#define LEDN_SL(C)                                                                                                     \
    do {                                                                                                               \
        const dim3 grid((unsigned)cdiv((long)N * hc * (wc / (v4 ? 4 : 1)), 256));                                      \
        if (v4 && crop_planar) LEDN_LAUNCH((slide_accumulate_kernel<C, 4, true>), grid, dim3(256), 0, s, canvas, crop, N, H, W, y1, x1, hc, wc);  \
        else if (v4) LEDN_LAUNCH((slide_accumulate_kernel<C, 4, false>), grid, dim3(256), 0, s, canvas, crop, N, H, W, y1, x1, hc, wc);       \
        else if (crop_planar) LEDN_LAUNCH((slide_accumulate_kernel<C, 1, true>), grid, dim3(256), 0, s, canvas, crop, N, H, W, y1, x1, hc, wc); \
        else LEDN_LAUNCH((slide_accumulate_kernel<C, 1, false>), grid, dim3(256), 0, s, canvas, crop, N, H, W, y1, x1, hc, wc);               \
    } while (0)
    switch (C) {
        case 2: LEDN_SL(2); break;
        case 3: LEDN_SL(3); break;
        case 4: LEDN_SL(4); break;
        case 5: LEDN_SL(5); break;
        case 8: LEDN_SL(8); break;
        case 19: LEDN_SL(19); break;
        default: return LEDN_EINVAL;
    }
#undef LEDN_SL
    return check_launch();
}

// ---- canvas[n, c, y, x] /= rowcnt[y] * colcnt[x] (the window count is the outer product of the two), first-max argmax ----
template <int C, int PX>
__global__ void __launch_bounds__(256) slide_finish_kernel(float* canvas, const int* rowcnt, const int* colcnt,
                                                           unsigned char* mask, int N, int H, int W) {
    const unsigned wq = (unsigned)(W / PX);
    const unsigned total = (unsigned)N * H * wq;
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const unsigned row = idx / wq, n = row / (unsigned)H;
    const int x = (int)(idx - row * wq) * PX, y = (int)(row - n * (unsigned)H);
    const long plane = (long)H * W, off = (long)y * W + x;
    float* cv = canvas + (long)n * C * plane + off;
    const int rc = rowcnt[y];
    float cnt[PX], bv[PX] = {};
    int best[PX] = {};
#pragma unroll
    for (int j = 0; j < PX; ++j) cnt[j] = (float)(rc * colcnt[x + j]);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float a[PX];
        ldpx<PX>(cv + c * plane, a);
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            a[j] = a[j] / cnt[j];
            if (c == 0 || a[j] > bv[j]) {
                bv[j] = a[j];
                best[j] = c;
            }
        }
        stpx<PX>(cv + c * plane, a);
    }
    if (mask) st_mask<PX>(mask + (long)n * plane + off, best);
}

int slide_finish_impl(float* canvas, const int* rowcnt, const int* colcnt, unsigned char* mask, int N, int C, int H,
                      int W, hipStream_t s) {
    LEDN_REQUIRE(canvas && rowcnt && colcnt && N > 0 && H > 0 && W > 0);
    LEDN_REQUIRE((long)N * C * H * W < 0x7fffffffL * 4L && (long)N * H * W < 0x7fffffffL);
    LEDN_REQUIRE(aligned(canvas, 4) && aligned(rowcnt, 4) && aligned(colcnt, 4));
    const bool v4 = W % 4 == 0 && aligned(canvas, 16) && (!mask || aligned(mask, 4));
    const dim3 grid((unsigned)cdiv((long)N * H * (W / (v4 ? 4 : 1)), 256));
#define LEDN_SF(C)                                                                                                    \
    do {                                                                                                              \
        if (v4) LEDN_LAUNCH((slide_finish_kernel<C, 4>), grid, dim3(256), 0, s, canvas, rowcnt, colcnt, mask, N, H, W); \
        else LEDN_LAUNCH((slide_finish_kernel<C, 1>), grid, dim3(256), 0, s, canvas, rowcnt, colcnt, mask, N, H, W);    \
    } while (0)
    switch (C) {
        case 2: LEDN_SF(2); break;
        case 3: LEDN_SF(3); break;
        case 4: LEDN_SF(4); break;
        case 5: LEDN_SF(5); break;
        case 8: LEDN_SF(8); break;
        case 19: LEDN_SF(19); break;
        default: return LEDN_EINVAL;
    }
#undef LEDN_SF
    return check_launch();
}

}  // namespace ledn
