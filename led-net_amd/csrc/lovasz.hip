// lovasz.hip -- LovaszLoss (multi-class Lovasz-Softmax, mmseg/models/losses/lovasz_loss.py:129-222) for LEDHead.
//
// Unlike the losses of seg_loss.hip this one needs the pixels of every class RANKED by their error, so the forward is a
// graph-capturable, bit-reproducible least-significant-digit radix sort of (key, pixel index) pairs and the Lovasz
// gradient on top of it.  Nothing here waits on another workgroup (no look-back, no flag): every dependency between
// workgroups is a kernel boundary, so the emulation build (workgroups one after another) runs the same sources.  No
// float atomics; the only atomics are integer counts.
//
// Segments: the ranking is over all valid pixels of the batch (S = 1 segment of L = N*HW pixels) or per image
// (per_image: S = N segments of L = HW).  A segment is cut into tiles of LV_TILE pixels, one workgroup each:
// grid (nblk, S), nblk = ceil(L / LV_TILE).  Classes run one after another through the same buffers.
//
// Per class c of the loss:
//   build    e = |fg - softmax(logits)_c| clamped to [0, 1], fg = (label == c); key = ((bits(e) << 1) | fg) + 1 (at most
//            LV_KEY_TOP: 31 bits; key 0 = ignored pixel) and the sort key sk = LV_KEY_TOP - key, so that ASCENDING sk is
//            descending error, then foreground first, and ignored pixels form one run at the very end; idx = pixel.
//   4 x      hist (digit counts per tile) -> scan (per digit, over the tiles; digit totals) -> scatter (stable: a wave
//            ranks its 64 elements by digit with ballots, waves and rounds in order; per-digit runs) -- 8-bit digits.
//            The sort is stable, so equal keys stay in pixel order: the tie order is error descending, foreground
//            first, lower pixel index first.
//   fgtot    foreground count of each tile of the sorted order -> scan -> F of the tile's first element
//   loss     at sorted position i with F / B foreground / background elements before it, G the class's foreground
//            count: U = G + B, I = G - F; g = 1 / U (foreground), I / (U (U + 1)) (background), 1 for U = 0 -- the
//            increment of the Jaccard index in closed form from exact integer counts (lovasz_grad, :15-27, without the
//            f32 difference of two nearly equal numbers).  Tile partial of sum e g (times class_weight[c]); g scattered
//            to gbuf[pixel].
//   accum    dlog[p][k] += w s g p_c (delta_ck - p_k), s = -1 (foreground) / +1; w = class_weight[c] (per_image: divided
//            by the number of classes computed for that image).  dlog is unscaled: the backward multiplies it by
//            dloss * loss_weight / out[2].
// 'present' (mode 1) skips a class without a foreground pixel in the segment: every kernel of that (segment, class)
// returns at once (the count is on the device, the launch sequence never depends on it).
//
// work (4-byte words; P = N*HW): hdr[4] = loss_weight, #correct, -, - | dlog[P][C] | key0[P] key1[P] idx0[P] idx1[P]
//   gbuf[P] (each of these six 16-byte aligned) | G[S][C] | valid[S] | nact[S] | closs[C][S] | lpart[C][S][nblk] |
//   hist[S][256][nblk] | dtot[S][256] | tfg[S][nblk].  dlog does not move with per_image: the backward needs no mode.
// out[4]: loss (loss_weight applied), accuracy in percent (the definition of seg_loss.hip), the divisor of the mean
// (per_image: N for 'mean', 1 for 'sum'; else the number of classes computed), the number of valid pixels.
// No valid pixel, or no class computed: loss 0, gradient 0.
#include "ledn_rt.h"

namespace ledn {

constexpr int LV_TILE = 2048;                 // elements one workgroup ranks per scatter (256 threads x 8)
constexpr int LV_ITEMS = LV_TILE / 256;
constexpr unsigned LV_KEY_TOP = 0x7F000002u;  // ((bits(1.0f) << 1) | 1) + 1
constexpr int LV_HDR = 4;
constexpr int LV_MAX_C = 1024;                // the per-workgroup class counts sit in LDS
constexpr float LV_F32_EPS = 1.1920929e-07f;
enum { LV_ALL = 0, LV_PRESENT = 1, LV_LIST = 2 };

struct LvLay {
    long S, L, nblk, P;
    long o_G, o_valid, o_nact, o_closs, o_lpart, o_hist, o_dtot, o_tfg, o_key0, o_key1, o_idx0, o_idx1, o_gbuf, o_dlog;
    long words;
};
static LvLay lv_layout(long N, long HW, int C, int per_image) {
    LvLay l;
    l.S = per_image ? N : 1;
    l.L = per_image ? HW : N * HW;
    l.nblk = cdiv(l.L, LV_TILE);
    l.P = N * HW;
    auto al = [](long v) { return (v + 3) & ~3L; };
    const long Pa = al(l.P);
    long o = LV_HDR;
    l.o_dlog = o;   o += al(l.P * C);
    l.o_key0 = o;   o += Pa;
    l.o_key1 = o;   o += Pa;
    l.o_idx0 = o;   o += Pa;
    l.o_idx1 = o;   o += Pa;
    l.o_gbuf = o;   o += Pa;
    l.o_G = o;      o += l.S * C;
    l.o_valid = o;  o += l.S;
    l.o_nact = o;   o += l.S;
    l.o_closs = o;  o += l.S * C;
    l.o_lpart = o;  o += (long)C * l.S * l.nblk;
    l.o_hist = o;   o += l.S * 256 * l.nblk;
    l.o_dtot = o;   o += l.S * 256;
    l.o_tfg = o;    o += l.S * l.nblk;
    l.words = o;
    return l;
}

long long lovasz_work_bytes(long long N, long long HW, int C, int per_image) {
    if (N <= 0 || HW <= 0 || C < 2 || C > LV_MAX_C || N * HW >= (1LL << 31)) return 0;
    return 4LL * lv_layout((long)N, (long)HW, C, per_image).words;
}

__device__ __forceinline__ unsigned lv_wave_sum_u(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// 'present': a class without a foreground pixel in the segment is not computed (the same answer in every thread of
// the workgroup: the kernels return on it before their first barrier)
__device__ __forceinline__ bool lv_active(const unsigned* G, int s, int C, int c, int mode) {
    return mode != LV_PRESENT || G[(long)s * C + c] != 0u;
}

// exclusive sum of v over the 256 threads (in thread order) and the total; s_a[2][256]; ends in a barrier
__device__ __forceinline__ unsigned lv_block_scan(unsigned v, unsigned (*s_a)[256], unsigned& total) {
    const int t = threadIdx.x;
    s_a[0][t] = v;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < 256; off <<= 1) {
        unsigned x = s_a[cur][t];
        if (t >= off) x += s_a[cur][t - off];
        s_a[cur ^ 1][t] = x;
        __syncthreads();
        cur ^= 1;
    }
    const unsigned incl = s_a[cur][t];
    total = s_a[cur][255];
    __syncthreads();
    return incl - v;
}

// ---------------------------------------------------------------------------------------------------------------
// once per call: foreground counts G[s][c] over the valid pixels, #valid per segment, #correct (accuracy)
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lv_count_kernel(const float* logits, const long long* target, long L, int C,
                                                       int ignore_index, unsigned* G, unsigned* valid, unsigned* correct) {
    LEDN_DYN_SHARED(unsigned, s_g);          // [C]
    __shared__ unsigned s_u[4][2];
    const int s = blockIdx.y, t = threadIdx.x;
    for (int c = t; c < C; c += 256) s_g[c] = 0u;
    __syncthreads();
    const long base = (long)s * L;
    unsigned nv = 0u, nc = 0u;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long i = (long)blockIdx.x * LV_TILE + j * 256 + t;
        if (i < L) {
            const long gp = base + i;
            const long long tg = target[gp];
            if (tg != ignore_index) {
                const float* lg = logits + gp * C;
                float mx = lg[0];
                int am = 0;
                for (int c = 1; c < C; ++c)
                    if (lg[c] > mx) { mx = lg[c]; am = c; }
                ++nv;
                if (am == tg) ++nc;
                if (tg >= 0 && tg < C) atomicAdd(&s_g[(int)tg], 1u);
            }
        }
    }
    nv = lv_wave_sum_u(nv);
    nc = lv_wave_sum_u(nc);
    if (lane_id() == 0) { s_u[t >> 6][0] = nv; s_u[t >> 6][1] = nc; }
    __syncthreads();
    for (int c = t; c < C; c += 256)
        if (s_g[c]) atomicAdd(&G[(long)s * C + c], s_g[c]);
    if (t == 0) {
        atomicAdd(&valid[s], s_u[0][0] + s_u[1][0] + s_u[2][0] + s_u[3][0]);
        atomicAdd(correct, s_u[0][1] + s_u[1][1] + s_u[2][1] + s_u[3][1]);
    }
}

// the number of classes computed in each segment
__global__ void __launch_bounds__(256) lv_prep_kernel(const unsigned* G, int S, int C, int mode, int nlist, float* nact) {
    for (int s = threadIdx.x; s < S; s += 256) {
        int n = mode == LV_LIST ? nlist : C;
        if (mode == LV_PRESENT) {
            n = 0;
            for (int c = 0; c < C; ++c) n += G[(long)s * C + c] != 0u ? 1 : 0;
        }
        nact[s] = (float)n;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// per class
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lv_build_kernel(const float* logits, const long long* target, long L, int C, int c,
                                                       int mode, int ignore_index, const unsigned* G, unsigned* key,
                                                       unsigned* idx) {
    const int s = blockIdx.y, t = threadIdx.x;
    if (!lv_active(G, s, C, c, mode)) return;
    const long base = (long)s * L;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long i = (long)blockIdx.x * LV_TILE + j * 256 + t;
        if (i >= L) continue;
        const long gp = base + i;
        const long long tg = target[gp];
        unsigned sk = LV_KEY_TOP;          // (ignored: key 0)
        if (tg != ignore_index) {
            const float* lg = logits + gp * C;
            float mx = lg[0];
            for (int k = 1; k < C; ++k) mx = fmaxf(mx, lg[k]);
            float se = 0.f;
            for (int k = 0; k < C; ++k) se += __expf(lg[k] - mx);
            const float p = __expf(lg[c] - mx) / se;
            const unsigned fg = tg == c ? 1u : 0u;
            const float e = fminf(fmaxf(fg ? 1.f - p : p, 0.f), 1.f);
            const unsigned bits = __float_as_uint(e) & 0x7fffffffu;          // (-0.0f -> 0)
            sk = LV_KEY_TOP - (((bits << 1) | fg) + 1u);
        }
        key[gp] = sk;
        idx[gp] = (unsigned)gp;
    }
}

__global__ void __launch_bounds__(256) lv_hist_kernel(const unsigned* key, long L, int shift, int C, int c, int mode,
                                                      const unsigned* G, unsigned* hist, int nblk) {
    __shared__ unsigned s_h[256];
    const int s = blockIdx.y, t = threadIdx.x, lane = lane_id();
    if (!lv_active(G, s, C, c, mode)) return;
    s_h[t] = 0u;
    __syncthreads();
    const long base = (long)s * L;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long i = (long)blockIdx.x * LV_TILE + j * 256 + t;
        const bool ok = i < L;
        const unsigned d = ok ? (key[base + i] >> shift) & 255u : 0u;
        const unsigned long long m = wave_match8(d, ok);          // one LDS add per digit and wave, not per element
        if (ok && (m & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&s_h[d], (unsigned)__popcll(m));
    }
    __syncthreads();
    hist[((long)s * 256 + t) * nblk + blockIdx.x] = s_h[t];
}

// one workgroup per row of n counts: exclusive scan in place, the row's total to totals[row]
__global__ void __launch_bounds__(256) lv_scan_kernel(unsigned* data, int n, unsigned* totals, int rows_per_seg, int C,
                                                      int c, int mode, const unsigned* G) {
    __shared__ unsigned s_a[2][256];
    const int row = blockIdx.x, t = threadIdx.x;
    if (!lv_active(G, row / rows_per_seg, C, c, mode)) return;
    unsigned* d = data + (long)row * n;
    const int per = (n + 255) / 256;
    const int lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    unsigned sum = 0u;
    for (int i = lo; i < hi; ++i) sum += d[i];
    unsigned total;
    unsigned run = lv_block_scan(sum, s_a, total);
    for (int i = lo; i < hi; ++i) {
        const unsigned v = d[i];
        d[i] = run;
        run += v;
    }
    if (totals && t == 0) totals[row] = total;
}

// stable scatter of one tile by the digit at `shift`.  Element order inside the tile: wave, round, lane (index
// w * 512 + r * 64 + lane): a wave's ballots give the rank among its 64 elements, its per-digit counter the elements of
// its earlier rounds, the counters of the earlier waves the rest.
__global__ void __launch_bounds__(256) lv_scatter_kernel(const unsigned* key_in, const unsigned* idx_in, unsigned* key_out,
                                                         unsigned* idx_out, long L, int shift, int C, int c, int mode,
                                                         const unsigned* G, const unsigned* hist, const unsigned* dtot,
                                                         int nblk) {
    __shared__ unsigned s_cnt[4][256];
    __shared__ unsigned s_a[2][256];
    __shared__ unsigned s_base[256];
    const int s = blockIdx.y, t = threadIdx.x, w = t >> 6, lane = lane_id();
    if (!lv_active(G, s, C, c, mode)) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) s_cnt[q][t] = 0u;
    __syncthreads();
    const long base = (long)s * L;
    unsigned k[LV_ITEMS], ix[LV_ITEMS], rank[LV_ITEMS];
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        const long i = (long)blockIdx.x * LV_TILE + w * (64 * LV_ITEMS) + r * 64 + lane;
        const bool ok = i < L;
        k[r] = ok ? key_in[base + i] : 0u;
        ix[r] = ok ? idx_in[base + i] : 0u;
        const unsigned d = (k[r] >> shift) & 255u;
        const unsigned long long m = wave_match8(d, ok);
        const unsigned below = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        const unsigned pre = ok ? s_cnt[w][d] : 0u;
        wave_sync();
        if (ok && below == 0u) s_cnt[w][d] = pre + (unsigned)__popcll(m);
        wave_sync();
        rank[r] = pre + below;
    }
    __syncthreads();
    {   // thread t = digit t: the waves' counts -> exclusive over the waves; the digit's first output position
        const unsigned c0 = s_cnt[0][t], c1 = s_cnt[1][t], c2 = s_cnt[2][t];
        unsigned total;
        const unsigned dbase = lv_block_scan(dtot[(long)s * 256 + t], s_a, total);
        s_cnt[0][t] = 0u;
        s_cnt[1][t] = c0;
        s_cnt[2][t] = c0 + c1;
        s_cnt[3][t] = c0 + c1 + c2;
        s_base[t] = dbase + hist[((long)s * 256 + t) * nblk + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LV_ITEMS; ++r) {
        const long i = (long)blockIdx.x * LV_TILE + w * (64 * LV_ITEMS) + r * 64 + lane;
        if (i < L) {
            const unsigned d = (k[r] >> shift) & 255u;
            const long pos = (long)s_base[d] + s_cnt[w][d] + rank[r];
            if (pos < L) {          // (always: the counts are those of hist; kept as the bound of the store)
                key_out[base + pos] = k[r];
                idx_out[base + pos] = ix[r];
            }
        }
    }
}

__device__ __forceinline__ unsigned lv_key_of(unsigned sk) { return LV_KEY_TOP - sk; }
__device__ __forceinline__ unsigned lv_fg_of(unsigned key) { return key != 0u ? (key - 1u) & 1u : 0u; }

__global__ void __launch_bounds__(256) lv_fgtot_kernel(const unsigned* key, long L, int C, int c, int mode,
                                                       const unsigned* G, unsigned* tfg, int nblk) {
    __shared__ unsigned s_u[4];
    const int s = blockIdx.y, t = threadIdx.x;
    if (!lv_active(G, s, C, c, mode)) return;
    const long base = (long)s * L;
    unsigned n = 0u;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long i = (long)blockIdx.x * LV_TILE + j * 256 + t;
        if (i < L) n += lv_fg_of(lv_key_of(key[base + i]));
    }
    n = lv_wave_sum_u(n);
    if (lane_id() == 0) s_u[t >> 6] = n;
    __syncthreads();
    if (t == 0) tfg[(long)s * nblk + blockIdx.x] = s_u[0] + s_u[1] + s_u[2] + s_u[3];
}

// the Lovasz gradient along the sorted order; thread t owns the LV_ITEMS consecutive elements from t * LV_ITEMS
__global__ void __launch_bounds__(256) lv_loss_kernel(const unsigned* key, const unsigned* idx, long L, int C, int c,
                                                      int mode, const unsigned* G, const unsigned* tfg, const float* cw,
                                                      float* gbuf, float* lpart, int nblk) {
    __shared__ unsigned s_a[2][256];
    __shared__ float s_f[4];
    const int s = blockIdx.y, t = threadIdx.x;
    if (!lv_active(G, s, C, c, mode)) return;
    const long base = (long)s * L, i0 = (long)blockIdx.x * LV_TILE + (long)t * LV_ITEMS;
    unsigned k[LV_ITEMS], cnt = 0u;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        k[j] = i0 + j < L ? lv_key_of(key[base + i0 + j]) : 0u;
        cnt += lv_fg_of(k[j]);
    }
    unsigned total;
    unsigned F = tfg[(long)s * nblk + blockIdx.x] + lv_block_scan(cnt, s_a, total);
    const unsigned Gc = G[(long)s * C + c];
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long i = i0 + j;
        if (i < L) {
            float g = 0.f;
            if (k[j] != 0u) {          // (ignored pixels: the last run of the order, error 0, no gradient)
                const unsigned k1 = k[j] - 1u, fg = k1 & 1u;
                const float e = __uint_as_float(k1 >> 1);
                const unsigned B = (unsigned)i - F, U = Gc + B, I = Gc - F;
                if (fg) g = 1.f / (float)U;
                else g = U == 0u ? 1.f : (float)I / ((float)U * (float)(U + 1u));
                acc += e * g;
                F += fg;
            }
            gbuf[idx[base + i]] = g;
        }
    }
    acc = wave_sum(acc);
    if (lane_id() == 0) s_f[t >> 6] = acc;
    __syncthreads();
    if (t == 0) lpart[(long)s * nblk + blockIdx.x] = (cw ? cw[c] : 1.f) * ((s_f[0] + s_f[1]) + (s_f[2] + s_f[3]));
}

__global__ void __launch_bounds__(256) lv_accum_kernel(const float* logits, const long long* target, long L, int C, int c,
                                                       int mode, int per_image, int ignore_index, const unsigned* G,
                                                       const float* nact, const float* cw, const float* gbuf, float* dlog) {
    const int s = blockIdx.y, t = threadIdx.x;
    if (!lv_active(G, s, C, c, mode)) return;
    float w = cw ? cw[c] : 1.f;
    if (per_image) w = nact[s] > 0.f ? w / nact[s] : 0.f;
    const long base = (long)s * L;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long i = (long)blockIdx.x * LV_TILE + j * 256 + t;
        if (i >= L) continue;
        const long gp = base + i;
        const long long tg = target[gp];
        if (tg == ignore_index) continue;
        const float* lg = logits + gp * C;
        float mx = lg[0];
        for (int k = 1; k < C; ++k) mx = fmaxf(mx, lg[k]);
        float se = 0.f;
        for (int k = 0; k < C; ++k) se += __expf(lg[k] - mx);
        const float inv = 1.f / se;
        const float pc = __expf(lg[c] - mx) * inv;
        const float a = w * (tg == c ? -1.f : 1.f) * gbuf[gp] * pc;
        float* dl = dlog + gp * C;
        for (int k = 0; k < C; ++k) dl[k] += a * ((k == c ? 1.f : 0.f) - __expf(lg[k] - mx) * inv);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// finish: ONE workgroup.  Every (class slot, segment) series of tile partials is added by one wave in a fixed order,
// then thread 0 forms the means in a fixed order and writes out[4]
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lv_finish_kernel(float* work, LvLay l, int C, int K, int mode, int per_image,
                                                        int reduction, float loss_weight, int N, float* out) {
    const unsigned* G = reinterpret_cast<const unsigned*>(work) + l.o_G;
    const unsigned* valid = reinterpret_cast<const unsigned*>(work) + l.o_valid;
    const float* nact = work + l.o_nact;
    const float* lpart = work + l.o_lpart;
    float* closs = work + l.o_closs;
    const int wid = threadIdx.x >> 6, lane = lane_id();
    const int S = (int)l.S, nblk = (int)l.nblk;
    for (long e = wid; e < (long)K * S; e += 4) {
        const int k = (int)(e / S), s = (int)(e % S);
        const bool act = mode != LV_PRESENT || G[(long)s * C + k] != 0u;          // ('present': slot k is class k)
        float a = 0.f;
        if (act)
            for (int b = lane; b < nblk; b += 64) a += lpart[((long)k * S + s) * nblk + b];
        a = wave_sum(a);
        if (lane == 0) closs[(long)k * S + s] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float total = 0.f;
    unsigned nvalid = 0u;
    for (int s = 0; s < S; ++s) {
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc += closs[(long)k * S + s];
        total += nact[s] > 0.f ? acc / nact[s] : 0.f;
        nvalid += valid[s];
    }
    const float div = per_image ? (reduction == 0 ? (float)N : 1.f) : nact[0];
    out[0] = loss_weight * (per_image && reduction == 0 ? total / (float)N : total);
    out[1] = ((float)reinterpret_cast<const unsigned*>(work)[1] + LV_F32_EPS) * (100.0f / ((float)nvalid + LV_F32_EPS));
    out[2] = div;
    out[3] = (float)nvalid;
    work[0] = loss_weight;
}

__global__ void __launch_bounds__(256) lv_bwd_kernel(const float* dlog, const float* hdr, const float* out,
                                                     const float* dloss, long n, float* dlogits) {
    const float k = out[2] > 0.f ? dloss[0] * hdr[0] / out[2] : 0.f;
    const long n4 = n >> 2, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(dlog)[i];
        reinterpret_cast<float4*>(dlogits)[i] = make_float4(v.x * k, v.y * k, v.z * k, v.w * k);
    }
    if (blockIdx.x == 0)
        for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) dlogits[i] = dlog[i] * k;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static bool lv_shape_ok(int N, long long HW, int C) {
    return N > 0 && N <= 65535 && HW > 0 && C >= 2 && C <= LV_MAX_C && (long long)N * HW < (1LL << 31) &&
           (long long)N * HW * C < (1LL << 40);
}

int lovasz_fwd_impl(const float* logits, const long long* target, int N, long long HW, int C, const float* cw,
                    const int* classes, int nlist, int mode, int per_image, int reduction, int ignore_index,
                    float loss_weight, float* work, float* out, hipStream_t s) {
    LEDN_REQUIRE(logits && target && work && out && lv_shape_ok(N, HW, C));
    LEDN_REQUIRE(mode >= LV_ALL && mode <= LV_LIST && (reduction == 0 || reduction == 1));
    LEDN_REQUIRE(((uintptr_t)work & 15) == 0);
    if (mode == LV_LIST) {
        LEDN_REQUIRE(classes && nlist > 0 && nlist <= C);
        for (int a = 0; a < nlist; ++a) {
            LEDN_REQUIRE(classes[a] >= 0 && classes[a] < C);
            for (int b = 0; b < a; ++b) LEDN_REQUIRE(classes[a] != classes[b]);
        }
    }
    per_image = per_image ? 1 : 0;
    const LvLay l = lv_layout(N, (long)HW, C, per_image);
    unsigned* wu = reinterpret_cast<unsigned*>(work);
    unsigned *G = wu + l.o_G, *valid = wu + l.o_valid, *hist = wu + l.o_hist, *dtot = wu + l.o_dtot, *tfg = wu + l.o_tfg;
    unsigned* key[2] = {wu + l.o_key0, wu + l.o_key1};
    unsigned* idx[2] = {wu + l.o_idx0, wu + l.o_idx1};
    float *nact = work + l.o_nact, *gbuf = work + l.o_gbuf, *dlog = work + l.o_dlog;
    // hdr and dlog (adjacent); the counts G and valid (adjacent)
    if (hipMemsetAsync(work, 0, sizeof(float) * (size_t)l.o_key0, s) != hipSuccess) return LEDN_ELAUNCH;
    if (hipMemsetAsync(G, 0, sizeof(unsigned) * (size_t)(l.o_nact - l.o_G), s) != hipSuccess) return LEDN_ELAUNCH;
    const dim3 grid((unsigned)l.nblk, (unsigned)l.S), blk(256);
    const int nblk = (int)l.nblk, S = (int)l.S;
    LEDN_LAUNCH(lv_count_kernel, grid, blk, sizeof(unsigned) * C, s, logits, target, l.L, C, ignore_index, G, valid, wu + 1);
    LEDN_LAUNCH(lv_prep_kernel, dim3(1), blk, 0, s, G, S, C, mode, nlist, nact);
    const int K = mode == LV_LIST ? nlist : C;
    for (int k = 0; k < K; ++k) {
        const int c = mode == LV_LIST ? classes[k] : k;
        LEDN_LAUNCH(lv_build_kernel, grid, blk, 0, s, logits, target, l.L, C, c, mode, ignore_index, G, key[0], idx[0]);
        for (int pass = 0; pass < 4; ++pass) {
            const int a = pass & 1, shift = 8 * pass;
            LEDN_LAUNCH(lv_hist_kernel, grid, blk, 0, s, key[a], l.L, shift, C, c, mode, G, hist, nblk);
            LEDN_LAUNCH(lv_scan_kernel, dim3((unsigned)(S * 256)), blk, 0, s, hist, nblk, dtot, 256, C, c, mode, G);
            LEDN_LAUNCH(lv_scatter_kernel, grid, blk, 0, s, key[a], idx[a], key[a ^ 1], idx[a ^ 1], l.L, shift, C, c, mode, G,
                        hist, dtot, nblk);
        }
        LEDN_LAUNCH(lv_fgtot_kernel, grid, blk, 0, s, key[0], l.L, C, c, mode, G, tfg, nblk);
        LEDN_LAUNCH(lv_scan_kernel, dim3((unsigned)S), blk, 0, s, tfg, nblk, (unsigned*)nullptr, 1, C, c, mode, G);
        LEDN_LAUNCH(lv_loss_kernel, grid, blk, 0, s, key[0], idx[0], l.L, C, c, mode, G, tfg, cw, gbuf,
                    work + l.o_lpart + (long)k * S * nblk, nblk);
        LEDN_LAUNCH(lv_accum_kernel, grid, blk, 0, s, logits, target, l.L, C, c, mode, per_image, ignore_index, G, nact, cw,
                    gbuf, dlog);
    }
    LEDN_LAUNCH(lv_finish_kernel, dim3(1), blk, 0, s, work, l, C, K, mode, per_image, reduction, loss_weight, N, out);
    return check_launch();
}

int lovasz_bwd_impl(const float* work, const float* out, const float* dloss, int N, long long HW, int C, float* dlogits,
                    hipStream_t s) {
    LEDN_REQUIRE(work && out && dloss && dlogits && lv_shape_ok(N, HW, C));
    LEDN_REQUIRE((((uintptr_t)work | (uintptr_t)dlogits) & 15) == 0);
    const LvLay l = lv_layout(N, (long)HW, C, 0);
    const long n = l.P * C;
    long g = cdiv(n >> 2, 256 * 4);
    if (g < 1) g = 1;
    if (g > 8192) g = 8192;
    LEDN_LAUNCH(lv_bwd_kernel, dim3((unsigned)g), dim3(256), 0, s, work + l.o_dlog, work, out, dloss, n, dlogits);
    return check_launch();
}

}  // namespace ledn
