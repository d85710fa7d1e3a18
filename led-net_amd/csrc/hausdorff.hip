// hausdorff.hip -- HuasdorffDisstanceLoss (mmseg/models/losses/huasdorff_distance_loss.py:14-156, the reference's spelling)
// for LEDHead, on an exact Euclidean distance transform computed on the device.
//
// The reference weighs each pixel's squared probability error by D = d_seg^2 + d_gt^2, the squared distances to the
// nearest background pixel of the mask M_seg = (argmax != 0) and of M_gt = (label != 0) (0 on background), which it gets
// from scipy on the host.  Here both maps are exact INTEGER squared distances from a separable transform:
//   column   one lane per (image, column), lanes along x: a down and an up sweep give g(x, y), the vertical distance to
//            the nearest background pixel of the column (a column without one: saturated), stored squared, HD_INF2 for
//            "none".  The masks are formed on the fly (labels; first-max argmax of the f32 logits) and never written.
//   row      one workgroup per (image, row, map), the row of g^2 in LDS: d2(x) = min_x' (x - x')^2 + g2(x').  Each lane
//            walks outwards from its pixel (dx = 1, 2, ..) while dx^2 < best, starting from best = g2(x): no x' with
//            (x - x')^2 >= best can improve the minimum, so this is exact, and background pixels stop at once.  In place
//            (the row is staged before the first store, and a workgroup owns its row).
//            A row whose minimum is still HD_INF2 belongs to an image without any background pixel (no column has one):
//            it gets (y + 1)^2 + x^2, scipy's answer for such a mask (the distance to a ghost pixel at row -1, column 0;
//            an artefact that is reproduced, not endorsed: DESIGN.md).  No flag, no atomic.
//   loss     one streaming pass: softmax, D = d2_seg + d2_gt (left in the work buffer for the backward), per-workgroup
//            f64 partials of sum D * sum_{i>=1} (p_i - y)^2, and the accuracy counts
//   finish   ONE workgroup adds the partials in a fixed order, in f64 (D reaches H^2 + W^2: an f32 sum of 16 M such terms
//            would lose the project's 1e-4), and writes out[4]
//   backward one streaming kernel: dlogit_k = s D p_k (a_k - sum_i a_i p_i), a_0 = 0, a_i = 2 (p_i - y)
// Nothing waits on another workgroup, there is no atomic at all and nothing is read by the host: the launch sequence
// depends on the sizes only and the result is the same bits in every run and mode.
//
// work (4-byte words; P = N*H*W, Pa = P rounded up to 4): hdr[4] = loss_weight, loss_weight / (C P), the loss's
// ignore_index (int), - | A[Pa] int32 (d2_seg, then D) | B[Pa] int32 (d2_gt) | lpart[nblk] f64 | cnt[nblk][2] u32.
// out[4]: loss, accuracy in percent (the definition of seg_loss.hip, over label != acc_ignore_index), the divisor C P,
// the number of those valid pixels.
// Limits: 2 <= C <= 32, W <= 8192 (the row in LDS), H^2 + W^2 < 2^30 (every squared distance, HD_INF2 + W^2 and D fit an
// int32), N <= 65535, P < 2^31.
#include "ledn_rt.h"

namespace ledn {

constexpr int HD_INF2 = 1 << 30;      // g^2 of a column without a background pixel
constexpr int HD_GINF = 1 << 16;      // the saturated vertical distance (more than any H)
constexpr int HD_MAX_W = 8192;
constexpr int HD_MAX_C = 32;
constexpr int HD_TILE = 2048;         // pixels per workgroup of the streaming passes (256 threads x 8)
constexpr int HD_ITEMS = HD_TILE / 256;
constexpr int HD_HDR = 4;
constexpr float HD_F32_EPS = 1.1920929e-07f;

struct HdLay {
    long P, nblk, o_a, o_b, o_lpart, o_cnt, words;
};
static HdLay hd_layout(long N, long H, long W) {
    HdLay l;
    l.P = N * H * W;
    l.nblk = cdiv(l.P, HD_TILE);
    const long Pa = (l.P + 3) & ~3L;
    long o = HD_HDR;
    l.o_a = o;      o += Pa;
    l.o_b = o;      o += Pa;
    l.o_lpart = o;  o += 2 * l.nblk;          // (f64: o is a multiple of 4 words here)
    l.o_cnt = o;    o += 2 * l.nblk;
    l.words = o;
    return l;
}

static bool hd_map_ok(long long N, long long H, long long W) {
    return N > 0 && N <= 65535 && H > 0 && W > 0 && W <= HD_MAX_W && H * H + W * W < (1LL << 30) &&
           N * H * W < (1LL << 31);
}

long long hausdorff_work_bytes(long long N, long long H, long long W, int C) {
    if (!hd_map_ok(N, H, W) || C < 2 || C > HD_MAX_C) return 0;
    return 4LL * hd_layout((long)N, (long)H, (long)W).words;
}

// ---------------------------------------------------------------------------------------------------------------
// column pass
// ---------------------------------------------------------------------------------------------------------------
// the up sweep of one column whose down sweep left the saturating distance to the background above (0 = background):
// -> g^2, HD_INF2 for a column without background
__device__ __forceinline__ void hd_col_up(int* gp, int H, int W) {
    int d = HD_GINF;
    for (int y = H - 1; y >= 0; --y) {
        int v = gp[(long)y * W];
        d = v == 0 ? 0 : min(d + 1, HD_GINF);
        v = min(v, d);
        gp[(long)y * W] = v >= HD_GINF ? HD_INF2 : v * v;
    }
}

__global__ void __launch_bounds__(64) hd_col_mask_kernel(const unsigned char* mask, int H, int W, int* g) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const long base = (long)blockIdx.y * H * W + x;
    const unsigned char* m = mask + base;
    int* gp = g + base;
    int d = HD_GINF;
    for (int y = 0; y < H; ++y) {
        d = m[(long)y * W] != 0 ? min(d + 1, HD_GINF) : 0;
        gp[(long)y * W] = d;
    }
    hd_col_up(gp, H, W);
}

// both masks of the loss: M_seg = (first-max argmax of the logits != 0) -> gs, M_gt = (label != 0 and != ignore_index) -> gg
__global__ void __launch_bounds__(64) hd_col_loss_kernel(const float* logits, const long long* target, int H, int W, int C,
                                                         int ignore_index, int* gs, int* gg) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const long base = (long)blockIdx.y * H * W + x;
    int ds = HD_GINF, dg = HD_GINF;
    for (int y = 0; y < H; ++y) {
        const long i = base + (long)y * W;
        const long long tg = target[i];
        const float* lg = logits + i * C;
        float mx = lg[0];
        bool fg = false;
        for (int c = 1; c < C; ++c)
            if (lg[c] > mx) { mx = lg[c]; fg = true; }
        ds = fg ? min(ds + 1, HD_GINF) : 0;
        dg = (tg != 0 && tg != ignore_index) ? min(dg + 1, HD_GINF) : 0;
        gs[i] = ds;
        gg[i] = dg;
    }
    hd_col_up(gs + base, H, W);
    hd_col_up(gg + base, H, W);
}

// ---------------------------------------------------------------------------------------------------------------
// row pass, in place: grid (H, N, maps); map z starts at maps + z * map_stride
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) hd_row_kernel(int* maps, long map_stride, int H, int W) {
    LEDN_DYN_SHARED(int, s_g);          // [W]
    __shared__ int s_min[4];
    const int y = blockIdx.x, t = threadIdx.x;
    int* row = maps + (long)blockIdx.z * map_stride + ((long)blockIdx.y * H + y) * W;
    int mn = HD_INF2;
    for (int x = t; x < W; x += 256) {
        const int v = row[x];
        s_g[x] = v;
        mn = min(mn, v);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mn = min(mn, __shfl_xor(mn, m));
    if (lane_id() == 0) s_min[t >> 6] = mn;
    __syncthreads();
    mn = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
    if (mn >= HD_INF2) {          // an image without a background pixel
        for (int x = t; x < W; x += 256) row[x] = (y + 1) * (y + 1) + x * x;
        return;
    }
    for (int x = t; x < W; x += 256) {
        int best = s_g[x];
        const int lo = x, hi = W - 1 - x, lim = max(lo, hi);
        for (int dx = 1; dx <= lim && dx * dx < best; ++dx) {
            const int d2 = dx * dx;
            if (dx <= lo) best = min(best, d2 + s_g[x - dx]);
            if (dx <= hi) best = min(best, d2 + s_g[x + dx]);
        }
        row[x] = best;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// loss forward, finish, backward
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) hd_loss_kernel(const float* logits, const long long* target, long P, int C,
                                                      int ignore_index, int acc_ignore_index, int* A, const int* B,
                                                      double* lpart, unsigned* cnt) {
    __shared__ double s_d[4];
    __shared__ unsigned s_u[4][2];
    const int t = threadIdx.x;
    double acc = 0.0;
    unsigned nv = 0u, nc = 0u;
#pragma unroll
    for (int j = 0; j < HD_ITEMS; ++j) {
        const long i = (long)blockIdx.x * HD_TILE + j * 256 + t;
        if (i < P) {
            const long long tg = target[i];
            const float yf = tg == ignore_index ? 0.f : (float)tg;
            const float* lg = logits + i * C;
            float mx = lg[0];
            int am = 0;
            for (int c = 1; c < C; ++c)
                if (lg[c] > mx) { mx = lg[c]; am = c; }
            float se = 0.f;
            for (int c = 0; c < C; ++c) se += __expf(lg[c] - mx);
            const float inv = 1.f / se;
            float sq = 0.f;
            for (int c = 1; c < C; ++c) {
                const float d = __expf(lg[c] - mx) * inv - yf;
                sq += d * d;
            }
            const int D = A[i] + B[i];
            A[i] = D;
            acc += (double)D * (double)sq;
            if (tg != acc_ignore_index) {
                ++nv;
                if (am == tg) ++nc;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        acc += __shfl_xor(acc, m);
        nv += __shfl_xor(nv, m);
        nc += __shfl_xor(nc, m);
    }
    if (lane_id() == 0) { s_d[t >> 6] = acc; s_u[t >> 6][0] = nv; s_u[t >> 6][1] = nc; }
    __syncthreads();
    if (t == 0) {
        lpart[blockIdx.x] = (s_d[0] + s_d[1]) + (s_d[2] + s_d[3]);
        cnt[2 * (long)blockIdx.x] = s_u[0][0] + s_u[1][0] + s_u[2][0] + s_u[3][0];
        cnt[2 * (long)blockIdx.x + 1] = s_u[0][1] + s_u[1][1] + s_u[2][1] + s_u[3][1];
    }
}

// ONE workgroup: thread t adds the partials t, t + 256, .. in order, thread 0 the 256 sums in order
__global__ void __launch_bounds__(256) hd_finish_kernel(float* work, HdLay l, int C, int ignore_index, float loss_weight,
                                                        float* out) {
    __shared__ double s_d[256];
    __shared__ unsigned s_u[256][2];
    const double* lpart = reinterpret_cast<const double*>(work + l.o_lpart);
    const unsigned* cnt = reinterpret_cast<const unsigned*>(work) + l.o_cnt;
    const int t = threadIdx.x;
    double a = 0.0;
    unsigned nv = 0u, nc = 0u;
    for (long b = t; b < l.nblk; b += 256) {
        a += lpart[b];
        nv += cnt[2 * b];
        nc += cnt[2 * b + 1];
    }
    s_d[t] = a;
    s_u[t][0] = nv;
    s_u[t][1] = nc;
    __syncthreads();
    if (t != 0) return;
    a = 0.0;
    nv = nc = 0u;
    for (int i = 0; i < 256; ++i) {
        a += s_d[i];
        nv += s_u[i][0];
        nc += s_u[i][1];
    }
    const double div = (double)C * (double)l.P, scale = (double)loss_weight / div;
    out[0] = (float)(a * scale);
    out[1] = ((float)nc + HD_F32_EPS) * (100.0f / ((float)nv + HD_F32_EPS));
    out[2] = (float)div;
    out[3] = (float)nv;
    work[0] = loss_weight;
    work[1] = (float)scale;
    reinterpret_cast<int*>(work)[2] = ignore_index;
}

__global__ void __launch_bounds__(256) hd_bwd_kernel(const float* logits, const long long* target, long P, int C,
                                                     const float* hdr, const int* Dm, const float* dloss, float* dlogits) {
    const float s = dloss[0] * hdr[1];
    const int ignore_index = reinterpret_cast<const int*>(hdr)[2];
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < HD_ITEMS; ++j) {
        const long i = (long)blockIdx.x * HD_TILE + j * 256 + t;
        if (i >= P) continue;
        const long long tg = target[i];
        const float yf = tg == ignore_index ? 0.f : (float)tg;
        const float* lg = logits + i * C;
        float mx = lg[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, lg[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf(lg[c] - mx);
        const float inv = 1.f / se;
        // a_k - sum_i a_i p_i without the difference of two numbers of size 2 y (y is the RAW label, up to 255):
        // with S1 = sum_{i>=1} p_i = 1 - p_0 and S2 = sum_{i>=1} p_i^2 it is 2 (p_k - S2 - y p_0) for k >= 1 and
        // 2 (y S1 - S2) for k = 0
        float s1 = 0.f, s2 = 0.f;
        for (int c = 1; c < C; ++c) {
            const float p = __expf(lg[c] - mx) * inv;
            s1 += p;
            s2 += p * p;
        }
        const float p0 = __expf(lg[0] - mx) * inv;
        const float k = 2.f * s * (float)Dm[i];
        float* dl = dlogits + i * C;
        dl[0] = k * p0 * (yf * s1 - s2);
        for (int c = 1; c < C; ++c) {
            const float p = __expf(lg[c] - mx) * inv;
            dl[c] = k * p * (p - s2 - yf * p0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int hd_rows(int* maps, long map_stride, int nmaps, int N, int H, int W, hipStream_t s) {
    LEDN_LAUNCH(hd_row_kernel, dim3((unsigned)H, (unsigned)N, (unsigned)nmaps), dim3(256), sizeof(int) * (size_t)W, s, maps,
                map_stride, H, W);
    return LEDN_OK;
}

int edt_sq_impl(const unsigned char* mask, int N, int H, int W, int* out, hipStream_t s) {
    LEDN_REQUIRE(mask && out && hd_map_ok(N, H, W));
    LEDN_LAUNCH(hd_col_mask_kernel, dim3((unsigned)cdiv(W, 64), (unsigned)N), dim3(64), 0, s, mask, H, W, out);
    hd_rows(out, 0, 1, N, H, W, s);
    return check_launch();
}

int hausdorff_fwd_impl(const float* logits, const long long* target, int N, int H, int W, int C, int ignore_index,
                       int acc_ignore_index, float loss_weight, float* work, float* out, hipStream_t s) {
    LEDN_REQUIRE(logits && target && work && out && hd_map_ok(N, H, W) && C >= 2 && C <= HD_MAX_C);
    LEDN_REQUIRE(((uintptr_t)work & 15) == 0);
    const HdLay l = hd_layout(N, H, W);
    int *A = reinterpret_cast<int*>(work) + l.o_a, *B = reinterpret_cast<int*>(work) + l.o_b;
    LEDN_LAUNCH(hd_col_loss_kernel, dim3((unsigned)cdiv(W, 64), (unsigned)N), dim3(64), 0, s, logits, target, H, W, C,
                ignore_index, A, B);
    hd_rows(A, l.o_b - l.o_a, 2, N, H, W, s);
    LEDN_LAUNCH(hd_loss_kernel, dim3((unsigned)l.nblk), dim3(256), 0, s, logits, target, l.P, C, ignore_index,
                acc_ignore_index, A, B, reinterpret_cast<double*>(work + l.o_lpart),
                reinterpret_cast<unsigned*>(work) + l.o_cnt);
    LEDN_LAUNCH(hd_finish_kernel, dim3(1), dim3(256), 0, s, work, l, C, ignore_index, loss_weight, out);
    return check_launch();
}

int hausdorff_bwd_impl(const float* logits, const long long* target, int N, int H, int W, int C, const float* work,
                       const float* dloss, float* dlogits, hipStream_t s) {
    LEDN_REQUIRE(logits && target && work && dloss && dlogits && hd_map_ok(N, H, W) && C >= 2 && C <= HD_MAX_C);
    const HdLay l = hd_layout(N, H, W);
    LEDN_LAUNCH(hd_bwd_kernel, dim3((unsigned)l.nblk), dim3(256), 0, s, logits, target, l.P, C, work,
                reinterpret_cast<const int*>(work) + l.o_a, dloss, dlogits);
    return check_launch();
}

}  // namespace ledn
