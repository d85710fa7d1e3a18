// stencil_bf16.hip -- vectorised bf16 kernels (see stencil.h) for the depthwise weight gradient
// and the SESP pyramid forward / data gradient / weight gradient.  Each returns -1 when the shape
// is outside its gate so that the caller (dwconv.hip / backward.hip) falls back to the generic kernel.
#include <cstdlib>
#include "stencil.h"

namespace ledn {

static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// sums `acc` (9 taps x 8 channels) over the pixel rows of one wave (lanes r*cvn + cv, cvn a power
// of two), then over the 4 waves through LDS; thread e < nine*C then owns element e of [9][C]
__device__ __forceinline__ void reduce_taps(f32x2_t (&acc)[9][4], int cvn, float* s_red /* [4][9*C] */, int C,
                                            int c) {
#define LEDN_RT_LEVEL(M)                                                        \
    if (cvn <= (M)) {                                                           \
        _Pragma("unroll") for (int t = 0; t < 9; ++t)                           \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                     \
                acc[t][i].x = lane_step_sum(acc[t][i].x, (M));                  \
                acc[t][i].y = lane_step_sum(acc[t][i].y, (M));                  \
            }                                                                   \
    }
    LEDN_RT_LEVEL(32)
    LEDN_RT_LEVEL(16)
    LEDN_RT_LEVEL(8)
    LEDN_RT_LEVEL(4)
    LEDN_RT_LEVEL(2)
    LEDN_RT_LEVEL(1)
#undef LEDN_RT_LEVEL
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane < cvn) {   // cvn <= 64: the first cvn lanes of the wave hold its sums (cvn == 64: one row per wave)
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s_red[(wid * 9 + t) * C + c + 2 * i] = acc[t][i].x;
                s_red[(wid * 9 + t) * C + c + 2 * i + 1] = acc[t][i].y;
            }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------
// depthwise 3x3 weight gradient: dw[t][c] = sum_pix x[pix @ tap t] * dz[pix]   (stride 1, pad = dil)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) dw3x3_bwd_weight_bf16_kernel(ledn_dwbwd_desc d, float* part) {
    constexpr int V = 8;
    LEDN_DYN_SHARED(float, s_red);   // [4][9*C]
    const int cvn = d.C / V;
    const int rows = 256 / cvn;
    const int r = threadIdx.x / cvn, cv = threadIdx.x % cvn;
    const int c = cv * V;
    f32x2_t acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[t][i] = f32x2_t{0.f, 0.f};
    {
        const int dl = d.dil[c / d.group_size];
        const bf16_t* x = reinterpret_cast<const bf16_t*>(d.x);
        const bf16_t* dz = reinterpret_cast<const bf16_t*>(d.dz);
        int toff[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) toff[t] = ((t / 3 - 1) * dl * d.W + (t % 3 - 1) * dl) * d.C;
        const long npix = (long)d.N * d.H * d.W;
        const long ppb = cdiv(cdiv(npix, (long)gridDim.x), (long)rows) * rows;
        const long p0 = (long)xcd_block(blockIdx.x, gridDim.x) * ppb, p1 = min(npix, p0 + ppb);
        PixCursor cur;
        cur.init(p0 + r, d.H, d.W);
        unsigned base = (unsigned)((p0 + r) * d.C + c);
        for (long p = p0 + r; p < p1; p += rows, base += (unsigned)(rows * d.C), cur.advance(rows, d.H, d.W)) {
            const unsigned mask = tap_mask(cur.y, cur.x, dl, d.H, d.W);
            uint4 raw[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) raw[t] = ld_tap(x, base + (unsigned)toff[t], base, (mask >> t) & 1u);
            f32x2_t g[4];
            bf16x8_unpack(*reinterpret_cast<const uint4*>(dz + base), g);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                f32x2_t xv[4];
                bf16x8_unpack(raw[t], xv);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[t][i] = pk_fma(xv[i], g[i], acc[t][i]);
            }
        }
    }
    reduce_taps(acc, cvn, s_red, d.C, c);
    for (int e = threadIdx.x; e < 9 * d.C; e += 256) {
        const float sum = (s_red[e] + s_red[9 * d.C + e]) + (s_red[18 * d.C + e] + s_red[27 * d.C + e]);
        if (part) part[(long)blockIdx.x * 9 * d.C + e] = sum;
        else atomicAdd(d.dw + e, sum);
    }
}

// the vectorised 3x3 weight gradient takes d (LEDN_DWBW_BF16_3X3): grid and ending
bool dw3x3_bwd_weight_bf16_plan(const ledn_dwbwd_desc& d, DwPlan* p) {   // used by backward.hip
    const int cvn = d.C / 8;
    if (d.dtype != LEDN_BF16 || d.KH != 3 || d.KW != 3 || d.stride != 1 || d.ext1 || d.C % 8 || d.group_size % 8 ||
        !pow2(cvn) || cvn > 64 || d.Ho != d.H || d.Wo != d.W || (long)d.N * d.H * d.W * d.C >= (1L << 31))
        return false;
    for (int g = 0; g * d.group_size < d.C; ++g)
        if (d.pad >= 0 && d.pad != d.dil[g]) return false;
    const int rows = 256 / cvn;
    // 16 pixels per thread (512 workgroups at 16 x 128 x 128 x 64): 28.8 / 36.6 us against 34.0 / 39.7 with 8 (graph replay,
    // r03); 32 and 64 are slower again.  Cost experiments of the same visit: every tap reading the centre pixel, only one tap
    // accumulated, next pixel's loads requested ahead -- none moved the time
    static const int ppt = (int)exp_knob("LEDN_DW_PPT", 16);     // (A/B knob)
    long nb = cdiv((long)d.N * d.H * d.W, rows * (ppt > 0 ? ppt : 16));
    if (nb > 1024) nb = 1024;
    float* part = (nb > 32 || det()) ? ws_take(nb * 9 * d.C) : nullptr;
    if (!part && nb > 128) nb = 128;
    p->kid = LEDN_DWBW_BF16_3X3;
    p->nb = p->rows = nb;
    p->part = part;
    return true;
}

int dw3x3_bwd_weight_bf16(const ledn_dwbwd_desc& d, const DwPlan& p, hipStream_t s) {   // used by backward.hip
    LEDN_LAUNCH(dw3x3_bwd_weight_bf16_kernel, dim3((unsigned)p.nb), dim3(256), (size_t)(36 * d.C) * sizeof(float), s, d,
                p.part);
    if (p.part) return finish_partials(p.part, (int)p.rows, 9 * d.C, 1, d.dw, nullptr, nullptr, s);
    return check_launch();
}

// ---------------------------------------------------------------------------
// SESP pyramid.  Weights [4][9][n] f32 sit in LDS (one copy per workgroup).
//   forward      : y[po][b*n + c] = sum_{b' <= b} dw3x3_{dil[b'], stride}(x)[po][c]
//   data gradient: dx[p][c] = sum_b sum_t g_b[p - tap_b(t)][c] * w[b][t][c]        (stride 1)
//   weight grad. : dw[b][t][c] = sum_po x[po*stride @ tap_b(t)][c] * g_b[po][c]
// ---------------------------------------------------------------------------
__device__ __forceinline__ void pyr_stage_weights(const float* w, float* s_w, int n) {
    for (int i = threadIdx.x; i < 36 * n; i += 256) s_w[i] = w[i];
    __syncthreads();
}

// SAME = all four dilations equal (the spatial branch: [1,1,1,1]): the four branches read the same nine taps, which
// are then loaded once instead of four times (the re-reads miss the vector L1 at 1/8 resolution and queue on the L2).
template <bool SAME>
__global__ void __launch_bounds__(256) pyr_fwd_bf16_kernel(ledn_pyr_desc d) {
    constexpr int V = 8;
    LEDN_DYN_SHARED(float, s_w);   // [36][n]
    pyr_stage_weights(d.w, s_w, d.n);
    const int cvn = d.n / V;
    const int rows = 256 / cvn;
    const int r = threadIdx.x / cvn, cv = threadIdx.x % cvn;
    const int c = cv * V;
    const bf16_t* x = reinterpret_cast<const bf16_t*>(d.x);
    bf16_t* y = reinterpret_cast<bf16_t*>(d.y);
    const long npo = (long)d.N * d.Ho * d.Wo;
    const long ppb = cdiv(cdiv(npo, (long)gridDim.x), (long)rows) * rows;
    const long p0 = (long)xcd_block(blockIdx.x, gridDim.x) * ppb, p1 = min(npo, p0 + ppb);
    PixCursor cur;
    cur.init(p0 + r, d.Ho, d.Wo);
    for (long p = p0 + r; p < p1; p += rows, cur.advance(rows, d.Ho, d.Wo)) {
        const int yi = cur.y * d.stride, xi = cur.x * d.stride;
        const unsigned base = (unsigned)((((long)cur.n * d.H + yi) * d.W + xi) * d.n + c);
        f32x2_t run[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) run[i] = f32x2_t{0.f, 0.f};
        uint4 raw[9];
        if (SAME) {
            const int dl = d.dil[0];
            const unsigned mask = tap_mask(yi, xi, dl, d.H, d.W);
            const int co = opaque(dl * d.n), ro = co * d.W;
#pragma unroll
            for (int t = 0; t < 9; ++t)
                raw[t] = ld_tap(x, base + (unsigned)((t / 3 - 1) * ro + (t % 3 - 1) * co), base, (mask >> t) & 1u);
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (!SAME) {
                const int dl = d.dil[b];
                const unsigned mask = tap_mask(yi, xi, dl, d.H, d.W);
                const int co = opaque(dl * d.n), ro = co * d.W;   // recomputed per pixel: 36 hoisted offsets cost a wave/SIMD
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    raw[t] = ld_tap(x, base + (unsigned)((t / 3 - 1) * ro + (t % 3 - 1) * co), base, (mask >> t) & 1u);
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                f32x2_t xv[4], wv[4];
                bf16x8_unpack(raw[t], xv);
                f32x8_load(s_w + (b * 9 + t) * d.n + c, wv);
#pragma unroll
                for (int i = 0; i < 4; ++i) run[i] = pk_fma(xv[i], wv[i], run[i]);
            }
            *reinterpret_cast<uint4*>(y + p * (4L * d.n) + (long)b * d.n + c) = bf16x8_pack(run);
            if (!SAME) sched_fence();   // one branch's nine taps in flight at a time (36 would cost the occupancy)
        }
    }
}

// the vectorised forward takes d: LEDN_PYR_BF16_SAME (four equal dilations) or LEDN_PYR_BF16
bool pyr_fwd_bf16_plan(const ledn_pyr_desc& d, DwPlan* p) {   // used by dwconv.hip
    const int cvn = d.n / 8;
    if (d.dtype_x != LEDN_BF16 || d.dtype_y != LEDN_BF16 || d.n % 8 || 256 % cvn || cvn > 256 ||
        (long)d.N * d.H * d.W * d.n * 4 >= (1L << 31))
        return false;
    const int rows = 256 / cvn;
    long nb = cdiv((long)d.N * d.Ho * d.Wo, rows * 2);
    if (nb > 2048) nb = 2048;
    p->kid = (d.dil[0] == d.dil[1] && d.dil[1] == d.dil[2] && d.dil[2] == d.dil[3]) ? LEDN_PYR_BF16_SAME : LEDN_PYR_BF16;
    p->nb = nb;
    return true;
}

int pyr_fwd_bf16(const ledn_pyr_desc& d, const DwPlan& p, hipStream_t s) {   // used by dwconv.hip
    const dim3 grid((unsigned)p.nb);
    if (p.kid == LEDN_PYR_BF16_SAME)
        LEDN_LAUNCH(pyr_fwd_bf16_kernel<true>, grid, dim3(256), (size_t)(36 * d.n) * sizeof(float), s, d);
    else
        LEDN_LAUNCH(pyr_fwd_bf16_kernel<false>, grid, dim3(256), (size_t)(36 * d.n) * sizeof(float), s, d);
    return check_launch();
}

// Equal dilations of 1 (the spatial branch), stride 1, large maps: the data gradient straight from dy with the
// PREFIX-summed filters  dx = sum_b corr(dy_b, flip(W_b)),  W_b = sum_{b' <= b} w_b'  -- no suffix-sum pass over dy
// (a launch that read and wrote all 4n channels) -- and with the dy patch staged ONCE in LDS: the gather kernel below
// issues 36 global 16-byte loads per output that miss the 32 KB vector L1 at 1/8 resolution and queue on the L2
// (85 us for 16 x 128 x 128, n = 32).  Workgroup = 128 lanes = a 8 x 32-pixel tile x 16 channels: patch
// [10 rows][4 branches][34 px][16 ch] (43.5 KB, three workgroups per CU), lane = (column, 8-channel group, 4 output
// rows): per branch the 9 x 8 filter values sit in registers and each of the 6 x 3 staged input pieces feeds up to
// three output rows (18 instead of 36 LDS reads per 4 outputs).
__global__ void __launch_bounds__(128) pyr_bwd_data_tile_kernel(ledn_pyrbwd_desc d) {
    constexpr int TW = 32, TH = 8, PW = TW + 2, PH = TH + 2;
    constexpr int NPIECE = PH * 4 * PW * 2;                 // 16-byte pieces: [py][b][px][half]
    constexpr int NL = (NPIECE + 127) / 128;
    __shared__ __attribute__((aligned(16))) unsigned char s_g[NPIECE * 16];
    __shared__ __attribute__((aligned(16))) float s_w[4 * 9 * 16];
    const int tid = threadIdx.x;
    const int tx = (d.W + TW - 1) / TW, ty = (d.H + TH - 1) / TH, nc = d.n / 16;
    const unsigned bid = xcd_block(blockIdx.x, gridDim.x);
    const int cgp = (int)(bid % (unsigned)nc);
    const unsigned tile = bid / (unsigned)nc;
    const int txi = (int)(tile % (unsigned)tx), tyi = (int)((tile / (unsigned)tx) % (unsigned)ty);
    const int img = (int)(tile / (unsigned)(tx * ty));
    const int c0 = cgp * 16, n4 = 4 * d.n;
    const bf16_t* dy = reinterpret_cast<const bf16_t*>(d.dy) + (long)img * d.H * d.W * n4 + c0;
    const int y0 = tyi * TH - 1, x0 = txi * TW - 1;
    {
        uint4 stage[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int e = tid + i * 128, half = e & 1, q = e >> 1;
            const int px = q % PW, rb = q / PW, b = rb & 3, py = rb >> 2;
            const int gy = y0 + py, gx = x0 + px;
            const bool ok = e < NPIECE && gy >= 0 && gy < d.H && gx >= 0 && gx < d.W;
            stage[i] = ok ? *reinterpret_cast<const uint4*>(dy + ((long)gy * d.W + gx) * n4 + b * d.n + half * 8)
                          : uint4{0u, 0u, 0u, 0u};
        }
        for (int i = tid; i < 9 * 16; i += 128) {           // prefix sums of the 16 channels' filters
            const int t = i >> 4, cc = i & 15;
            float run = 0.f;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                run += d.w[(long)(b * 9 + t) * d.n + c0 + cc];
                s_w[(b * 9 + t) * 16 + cc] = run;
            }
        }
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int e = tid + i * 128;
            if (e < NPIECE) *reinterpret_cast<uint4*>(s_g + (long)e * 16) = stage[i];
        }
    }
    __syncthreads();
    const int cg = tid & 1, lx = (tid >> 1) & 31, yg = tid >> 6;
    f32x2_t acc[4][4];
#pragma unroll
    for (int yo = 0; yo < 4; ++yo)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[yo][i] = f32x2_t{0.f, 0.f};
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
        f32x2_t w[9][4];
#pragma unroll
        for (int t = 0; t < 9; ++t) f32x8_load(s_w + (b * 9 + t) * 16 + cg * 8, w[t]);
#pragma unroll
        for (int r = 0; r < 6; ++r) {                        // staged row yg*4 + r = image row (first output row) - 1 + r
            const unsigned char* row = s_g + ((long)((yg * 4 + r) * 4 + b) * PW + lx) * 32 + cg * 16;
            f32x2_t in[3][4];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) bf16x8_unpack(*reinterpret_cast<const uint4*>(row + kx * 32), in[kx]);
#pragma unroll
            for (int yo = 0; yo < 4; ++yo) {
                const int ky = r - yo;                       // dx[y] += dy[y + ky - 1][x + kx - 1] * W[(2-ky)*3 + (2-kx)]
                if (ky < 0 || ky > 2) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[yo][i] = pk_fma(in[kx][i], w[8 - (ky * 3 + kx)][i], acc[yo][i]);
            }
        }
    }
    const int gx = txi * TW + lx;
    bf16_t* dx = reinterpret_cast<bf16_t*>(d.dx) + (long)img * d.H * d.W * d.n + c0 + cg * 8;
#pragma unroll
    for (int yo = 0; yo < 4; ++yo) {
        const int gy = tyi * TH + yg * 4 + yo;
        if (gy < d.H && gx < d.W) *reinterpret_cast<uint4*>(dx + ((long)gy * d.W + gx) * d.n) = bf16x8_pack(acc[yo]);
    }
}

// the tiled data gradient applies (and then nothing reads or writes gsum: the weight gradient forms its suffix sums
// from dy on the fly -- both entry points decide with this predicate)
bool pyr_tile_applies(const ledn_pyrbwd_desc& d) {
    return (options().stream_fast & 2) && d.dtype == LEDN_BF16 && d.stride == 1 && d.n % 16 == 0 && d.n <= 512 &&
           ((d.n / 8) & (d.n / 8 - 1)) == 0 && d.W >= 32 &&   // (n / 8 a power of two: the bf16 weight-gradient kernel's gate)
           d.dil[0] == 1 && d.dil[1] == 1 && d.dil[2] == 1 && d.dil[3] == 1 && (long)d.N * d.H * d.W >= 16384 &&
           (long)d.N * d.H * d.W * d.n * 4 < (1L << 31);
}

int pyr_bwd_data_tile(const ledn_pyrbwd_desc& d, hipStream_t s) {
    const long nb = (long)d.N * cdiv(d.H, 8) * cdiv(d.W, 32) * (d.n / 16);
    LEDN_LAUNCH(pyr_bwd_data_tile_kernel, dim3((unsigned)nb), dim3(128), 0, s, d);
    return check_launch();
}

// Unequal dilations (the context branch: [1,2,3,4]), stride 1 or 2, any map size: the data gradient straight from dy
// with the dy patch staged ONCE in LDS -- no suffix-sum launch, no gsum, none of the 36 global tap loads per output.
// Workgroup = 256 lanes = a 16 x 16-pixel tile of dy (= 16 S x 16 S pixels of dx) x 16 channels.  Branch b keeps its own
// patch [16 + 2 h_b]^2 x 16 channels with halo h_b = dil_b (stride 1) or ceil(dil_b / 2) (stride 2): for [1,2,3,4]
// 1784 pixels x 32 B = 55.75 KB at stride 1 (two workgroups per CU), 1448 pixels = 45.25 KB at stride 2 (three).  The
// lane that stages a dy pixel loads the pieces of the branches that need it (a pixel r rings outside the tile serves
// only the branches with h_b >= r, and the suffix sum of branch b needs only dy_b .. dy_3; all of a lane's up to 20
// loads are in flight together), forms g_b = sum_{b' >= b} dy_b' in f32 and stores it rounded to bf16 -- bit for bit
// what pyr_suffix_kernel leaves in gsum.  Gather: lane = (column, 8-channel group, 2 tile rows); per (branch, tap) the 8
// filter values are read once from LDS and feed both rows.  Stride 2: the four parities of dx are handled one after
// another (wave-uniform), each accumulating only the taps the stride leaves on the lattice (20 / 4 / 4 / 8 of 36 for
// [1,2,3,4]); a tap's offset in the patch is a constant of (parity, tap), no division per element.
// The taps are accumulated in the order of the kernels this one replaces (pyr_bwd_data_bf16_kernel at stride 1,
// pyr_bwd_data_kernel at stride 2), so dx is bit-identical to theirs.
// 128 lanes x 4 rows (one wave per SIMD) with the staging in three dependent rounds ran at 66 us where this form takes 50
// (16 x 128 x 128 x 32, stride 1); before the reads of a tap group were issued together it took 78.
constexpr int PYC_T = 16;
constexpr int PYC_MAXPIX1 = 1784, PYC_MAXPIX2 = 1448;    // patch pixels of [1,2,3,4]: halos 1,2,3,4 / 1,1,2,2
static __host__ __device__ __forceinline__ int pyc_halo(int dl, int stride) { return stride == 1 ? dl : (dl + 1) / 2; }

template <int S>
__global__ void __launch_bounds__(256) pyr_bwd_data_ctx_kernel(ledn_pyrbwd_desc d) {
    constexpr int T = PYC_T, NT = 256, R = 2, NB = 5;   // lanes, tile rows per lane, staged pieces in flight per lane
    __shared__ __attribute__((aligned(16))) unsigned char s_g[(S == 1 ? PYC_MAXPIX1 : PYC_MAXPIX2) * 32];   // per branch [row][column][half] x 16 B
    __shared__ __attribute__((aligned(16))) float s_w[36 * 16];
    const int tid = threadIdx.x;
    const int cw = d.n % 16 == 0 ? 16 : 8, nc = d.n / cw;       // channels per workgroup
    const int tx = (d.Wo + T - 1) / T, ty = (d.Ho + T - 1) / T;
    const unsigned bid = xcd_block(blockIdx.x, gridDim.x);
    const int cgp = (int)(bid % (unsigned)nc);
    const unsigned tile = bid / (unsigned)nc;
    const int txi = (int)(tile % (unsigned)tx), tyi = (int)((tile / (unsigned)tx) % (unsigned)ty);
    const int img = (int)(tile / (unsigned)(tx * ty));
    const int c0 = cgp * cw, n4 = 4 * d.n;
    int hb[4], pw[4], pb[4], hm = 0;
    {
        int run = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            hb[b] = pyc_halo(d.dil[b], S);
            pw[b] = T + 2 * hb[b];
            pb[b] = run;
            run += pw[b] * pw[b];
            hm = max(hm, hb[b]);
        }
    }
    const int pm = T + 2 * hm, nitem = pm * pm * 2;
    const int cy0 = tyi * T, cx0 = txi * T;
    const bf16_t* dy = reinterpret_cast<const bf16_t*>(d.dy) + (long)img * d.Ho * d.Wo * n4 + c0;
    for (int i = tid; i < 36 * 16; i += NT) {
        const int cc = i & 15;
        s_w[i] = cc < cw ? d.w[(long)(i >> 4) * d.n + c0 + cc] : 0.f;
    }
#pragma unroll 1
    for (int e0 = tid; e0 < nitem; e0 += NB * NT) {      // (one pass: 1152 pieces at halo 4)
        uint4 raw[NB][4];
        int mr[NB], mq[NB];                                   // ring of the staged pixel (-1: nothing to do), patch position
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int e = e0 + i * NT, half = e & 1, q = e >> 1;
            const int py = q / pm, px = q - py * pm;
            const int gy = cy0 - hm + py, gx = cx0 - hm + px;
            const int r = max(max(max(cy0 - gy, gy - (cy0 + T - 1)), max(cx0 - gx, gx - (cx0 + T - 1))), 0);
            int bmin = 4;
#pragma unroll
            for (int b = 3; b >= 0; --b)
                if (hb[b] >= r) bmin = b;
            const bool act = e < nitem && half * 8 < cw && bmin < 4;
            const bool ok = act && gy >= 0 && gy < d.Ho && gx >= 0 && gx < d.Wo;
            const bf16_t* src = dy + ((long)gy * d.Wo + gx) * n4 + half * 8;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                raw[i][b] = (ok && b >= bmin) ? *reinterpret_cast<const uint4*>(src + b * d.n) : uint4{0u, 0u, 0u, 0u};
            mr[i] = act ? r : -1;
            mq[i] = (py << 8) | (px << 1) | half;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (mr[i] < 0) continue;
            const int half = mq[i] & 1, px = (mq[i] >> 1) & 127, py = mq[i] >> 8;
            f32x2_t run[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) run[k] = f32x2_t{0.f, 0.f};
#pragma unroll
            for (int b = 3; b >= 0; --b) {
                f32x2_t tv[4];
                bf16x8_unpack(raw[i][b], tv);
#pragma unroll
                for (int k = 0; k < 4; ++k) run[k] += tv[k];
                if (hb[b] >= mr[i]) {
                    const int row = py - hm + hb[b], col = px - hm + hb[b];
                    *reinterpret_cast<uint4*>(s_g + ((long)(pb[b] + row * pw[b] + col) * 2 + half) * 16) = bf16x8_pack(run);
                }
            }
        }
    }
    __syncthreads();
    const int cg = tid & 1, lx = (tid >> 1) & 15, yg = tid >> 5;   // 8 row groups of R rows
    if (cg * 8 >= cw) return;
    bf16_t* dx = reinterpret_cast<bf16_t*>(d.dx) + (long)img * d.H * d.W * d.n + c0 + cg * 8;
#pragma unroll 1
    for (int cls = 0; cls < S * S; ++cls) {
        const int py = cls / S, px = cls % S;               // parity of the dx pixels of this pass
        f32x2_t acc[R][4];
#pragma unroll
        for (int yo = 0; yo < R; ++yo)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[yo][i] = f32x2_t{0.f, 0.f};
        int pbb = 0;
#pragma unroll 1
        for (int b = 0; b < 4; ++b) {                       // (a real loop: unrolled, the FMA chains sink below all 144 reads)
            const int dl = d.dil[b], hbb = pyc_halo(dl, S), pwb = T + 2 * hbb;
            const unsigned char* pbase = s_g + ((long)(pbb + (yg * R + hbb) * pwb + lx + hbb) * 2 + cg) * 16;
            const float* wb = s_w + b * 9 * 16 + cg * 8;
            // the reads of one group of taps (a filter row at stride 1, one tap at stride 2, where the lattice test is
            // per tap) are issued together, then consumed: left to itself the compiler waits for every read in turn
            // (216 LDS round trips per lane with one wave per SIMD to hide them)
            constexpr int G = S == 1 ? 3 : 1;
#pragma unroll
            for (int t0 = 0; t0 < 9; t0 += G) {
                if (S == 2) {
                    const int th = py - (t0 / 3 - 1) * dl, tw = px - (t0 % 3 - 1) * dl;
                    if ((th | tw) & 1) continue;                                 // off the stride's lattice (wave-uniform)
                }
                uint4 rg[G][R];
                f32x2_t wv[G][4];
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const int t = t0 + j, kh = S == 1 ? 2 - t / 3 : t / 3, kw = S == 1 ? 2 - t % 3 : t % 3;
                    const int oh = (py - (kh - 1) * dl) / S, ow = (px - (kw - 1) * dl) / S;   // dy pixel = tile pixel + (oh, ow)
                    const unsigned char* p = pbase + (oh * pwb + ow) * 32;
#pragma unroll
                    for (int yo = 0; yo < R; ++yo) rg[j][yo] = *reinterpret_cast<const uint4*>(p + yo * pwb * 32);
                    f32x8_load(wb + (kh * 3 + kw) * 16, wv[j]);
                }
                sched_fence();
#pragma unroll
                for (int j = 0; j < G; ++j)
#pragma unroll
                    for (int yo = 0; yo < R; ++yo) {
                        f32x2_t gv[4];
                        bf16x8_unpack(rg[j][yo], gv);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[yo][i] = pk_fma(gv[i], wv[j][i], acc[yo][i]);
                    }
                sched_fence();
            }
            pbb += pwb * pwb;
        }
        const int gx = (cx0 + lx) * S + px;
#pragma unroll
        for (int yo = 0; yo < R; ++yo) {
            const int gy = (cy0 + yg * R + yo) * S + py;
            if (gy < d.H && gx < d.W) *reinterpret_cast<uint4*>(dx + ((long)gy * d.W + gx) * d.n) = bf16x8_pack(acc[yo]);
        }
    }
}

// the context-branch tile kernel applies (like pyr_tile_applies: gsum is then neither written nor read).  Dilations in
// any order; the patches of the four branches must fit the LDS image sized for [1,2,3,4] at stride 1.
bool pyr_ctx_applies(const ledn_pyrbwd_desc& d) {
    if (!(options().stream_fast & 2) || d.dtype != LEDN_BF16 || d.n % 8 || !pow2(d.n / 8) || d.n > 512 ||
        (long)d.N * d.H * d.W * d.n * 4 >= (1L << 31) || pyr_tile_applies(d))
        return false;
    int pix = 0;
    for (int b = 0; b < 4; ++b) {
        const int h = pyc_halo(d.dil[b], d.stride);
        if (h > 4) return false;
        pix += (PYC_T + 2 * h) * (PYC_T + 2 * h);
    }
    return pix <= (d.stride == 1 ? PYC_MAXPIX1 : PYC_MAXPIX2);
}

int pyr_bwd_data_ctx(const ledn_pyrbwd_desc& d, hipStream_t s) {
    const long nb = (long)d.N * cdiv(d.Ho, PYC_T) * cdiv(d.Wo, PYC_T) * (d.n / (d.n % 16 == 0 ? 16 : 8));
    if (d.stride == 1) LEDN_LAUNCH(pyr_bwd_data_ctx_kernel<1>, dim3((unsigned)nb), dim3(256), 0, s, d);
    else LEDN_LAUNCH(pyr_bwd_data_ctx_kernel<2>, dim3((unsigned)nb), dim3(256), 0, s, d);
    return check_launch();
}

// one of the two tiled data gradients served the call: no gsum, the weight gradient forms its suffix sums from dy
bool pyr_from_dy(const ledn_pyrbwd_desc& d) { return pyr_tile_applies(d) || pyr_ctx_applies(d); }

// gsum holds the suffix sums g_b = sum_{b' >= b} dy_b' (pyr_suffix_kernel)
__global__ void __launch_bounds__(256) pyr_bwd_data_bf16_kernel(ledn_pyrbwd_desc d) {
    constexpr int V = 8;
    LEDN_DYN_SHARED(float, s_w);   // [36][n]
    pyr_stage_weights(d.w, s_w, d.n);
    const int cvn = d.n / V;
    const int rows = 256 / cvn;
    const int r = threadIdx.x / cvn, cv = threadIdx.x % cvn;
    const int c = cv * V;
    const bf16_t* g = reinterpret_cast<const bf16_t*>(d.gsum);
    bf16_t* dx = reinterpret_cast<bf16_t*>(d.dx);
    const long npix = (long)d.N * d.H * d.W;
    const long ppb = cdiv(cdiv(npix, (long)gridDim.x), (long)rows) * rows;
    const long p0 = (long)xcd_block(blockIdx.x, gridDim.x) * ppb, p1 = min(npix, p0 + ppb);
    PixCursor cur;
    cur.init(p0 + r, d.H, d.W);
    const int n4 = 4 * d.n;
    for (long p = p0 + r; p < p1; p += rows, cur.advance(rows, d.H, d.W)) {
        const unsigned base = (unsigned)(p * n4 + c);
        f32x2_t acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = f32x2_t{0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int dl = d.dil[b];
            const unsigned mask = tap_mask(cur.y, cur.x, dl, d.H, d.W);
            const int co = opaque(dl * n4), ro = co * d.W;
            uint4 raw[9];
#pragma unroll
            for (int t = 0; t < 9; ++t)   // source pixel of tap t is p - tap offset: mirrored index 8 - t
                raw[t] = ld_tap(g, base + (unsigned)(b * d.n) + (unsigned)((t / 3 - 1) * ro + (t % 3 - 1) * co), base,
                                (mask >> t) & 1u);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                f32x2_t gv[4], wv[4];
                bf16x8_unpack(raw[t], gv);
                f32x8_load(s_w + (b * 9 + (8 - t)) * d.n + c, wv);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = pk_fma(gv[i], wv[i], acc[i]);
            }
            sched_fence();
        }
        *reinterpret_cast<uint4*>(dx + p * d.n + c) = bf16x8_pack(acc);
    }
}

bool pyr_bwd_data_bf16_applies(const ledn_pyrbwd_desc& d) {   // also read by pyr_bwd_data_kernel_id (backward.hip)
    const int cvn = d.n / 8;
    return !(d.dtype != LEDN_BF16 || d.stride != 1 || d.n % 8 || 256 % cvn || cvn > 256 ||
             (long)d.N * d.H * d.W * d.n * 4 >= (1L << 31));
}

int pyr_bwd_data_bf16(const ledn_pyrbwd_desc& d, hipStream_t s) {   // gsum already holds the suffix sums
    if (!pyr_bwd_data_bf16_applies(d)) return -1;
    const int rows = 256 / (d.n / 8);
    long nb = cdiv((long)d.N * d.H * d.W, rows * 2);
    if (nb > 2048) nb = 2048;
    LEDN_LAUNCH(pyr_bwd_data_bf16_kernel, dim3((unsigned)nb), dim3(256), (size_t)(36 * d.n) * sizeof(float), s, d);
    return check_launch();
}

__global__ void __launch_bounds__(256) pyr_bwd_weight_bf16_kernel(ledn_pyrbwd_desc d, float* part, bool from_dy) {
    constexpr int V = 8;
    LEDN_DYN_SHARED(float, s_red);   // [4][9*n]
    const int b = blockIdx.y;
    const int dl = d.dil[b];
    const int cvn = d.n / V;
    const int rows = 256 / cvn;
    const int r = threadIdx.x / cvn, cv = threadIdx.x % cvn;
    const int c = cv * V;
    f32x2_t acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[t][i] = f32x2_t{0.f, 0.f};
    {
        const bf16_t* x = reinterpret_cast<const bf16_t*>(d.x);
        const bf16_t* g = reinterpret_cast<const bf16_t*>(from_dy ? d.dy : d.gsum);
        const long npo = (long)d.N * d.Ho * d.Wo;
        const long ppb = cdiv(cdiv(npo, (long)gridDim.x), (long)rows) * rows;
        const long p0 = (long)xcd_block(blockIdx.x, gridDim.x) * ppb, p1 = min(npo, p0 + ppb);
        PixCursor cur;
        cur.init(p0 + r, d.Ho, d.Wo);
        for (long p = p0 + r; p < p1; p += rows, cur.advance(rows, d.Ho, d.Wo)) {
            const int yi = cur.y * d.stride, xi = cur.x * d.stride;
            const unsigned base = (unsigned)((((long)cur.n * d.H + yi) * d.W + xi) * d.n + c);
            const unsigned mask = tap_mask(yi, xi, dl, d.H, d.W);
            uint4 raw[9];
#pragma unroll
            for (int t = 0; t < 9; ++t)
                raw[t] = ld_tap(x, base + (unsigned)(((t / 3 - 1) * dl * d.W + (t % 3 - 1) * dl) * d.n), base,
                                (mask >> t) & 1u);
            f32x2_t gv[4];
            if (from_dy) {      // g_b = sum_{b' >= b} dy_b' formed here (the tiled data gradient leaves no gsum behind)
#pragma unroll
                for (int i = 0; i < 4; ++i) gv[i] = f32x2_t{0.f, 0.f};
                // four unconditional loads in flight with the nine taps (a branch below b re-reads piece b and counts as
                // zero): 2 - 3 us per launch faster than a loop of 4 - b dependent trips on the context branch's shapes
                const unsigned gb = (unsigned)(p * (4L * d.n) + c);
                uint4 rw[4];
#pragma unroll
                for (int bb = 0; bb < 4; ++bb)
                    rw[bb] = ld_tap(g, gb + (unsigned)(bb * d.n), gb + (unsigned)(b * d.n), bb >= b);
#pragma unroll
                for (int bb = 3; bb >= 0; --bb) {
                    f32x2_t tv[4];
                    bf16x8_unpack(rw[bb], tv);
#pragma unroll
                    for (int i = 0; i < 4; ++i) gv[i] += tv[i];
                }
            } else {
                bf16x8_unpack(*reinterpret_cast<const uint4*>(g + p * (4L * d.n) + (long)b * d.n + c), gv);
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                f32x2_t xv[4];
                bf16x8_unpack(raw[t], xv);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[t][i] = pk_fma(xv[i], gv[i], acc[t][i]);
            }
        }
    }
    reduce_taps(acc, cvn, s_red, d.n, c);
    for (int e = threadIdx.x; e < 9 * d.n; e += 256) {
        const float sum = (s_red[e] + s_red[9 * d.n + e]) + (s_red[18 * d.n + e] + s_red[27 * d.n + e]);
        // dw layout [4][3][3][n]; partial layout [blk][4*9*n]
        if (part) part[(long)blockIdx.x * 36 * d.n + (long)b * 9 * d.n + e] = sum;
        else atomicAdd(d.dw + (long)b * 9 * d.n + e, sum);
    }
}

// The same gradient when all four branches share one dilation (the spatial SESP blocks: eesp.py:40-62 with Spatial=True)
// and the tiled data gradient left no suffix sums behind: ONE pass over the pixels for the four branches instead of one
// workgroup column per branch -- the nine taps of x are the same for every branch, so a lane loads them once (and the four
// dy vectors once) and feeds 4 x 9 accumulators per channel.  Lane = 4 channels of a pixel (8-byte loads; 144 f32
// accumulators, two waves per SIMD), next pixel's 13 loads in flight under the 72 packed FMAs of this one.  The branch-per-
// column kernel read x through the texture path 36 times and dy 10 times (386 MB for a 42 MB problem at n = 16) with
// nothing in flight while it computed: 40 us at 16 x 128 x 128 x 16.
// Epilogue: reduce-scatter over the two wave halves and the two rows of each half (v_permlane32_swap / v_permlane16_swap:
// one swap + one add per register PAIR, 144 -> 36 registers), a butterfly inside the 16-lane row for the rest.
__global__ void __launch_bounds__(256, 2) pyr_bwd_weight_same_kernel(ledn_pyrbwd_desc d, float* part) {
    constexpr int V = 4;
    LEDN_DYN_SHARED(float, s_red);   // [4 waves][36][n]
    const int dl = d.dil[0], n = d.n;
    const int cvn = n / V;           // 4, 8 or 16 lanes per pixel
    const int rows = 256 / cvn;
    const int r = threadIdx.x / cvn, cv = threadIdx.x % cvn;
    const int c = cv * V;
    // acc[(b * 9 + t) * 2 + i]: branch b, tap t, channel pair i
    f32x2_t acc[72];
#pragma unroll
    for (int j = 0; j < 72; ++j) acc[j] = f32x2_t{0.f, 0.f};
    {
        const bf16_t* x = reinterpret_cast<const bf16_t*>(d.x);
        const bf16_t* g = reinterpret_cast<const bf16_t*>(d.dy);
        int toff[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) toff[t] = ((t / 3 - 1) * dl * d.W + (t % 3 - 1) * dl) * n;
        const long npix = (long)d.N * d.H * d.W;
        const long ppb = cdiv(cdiv(npix, (long)gridDim.x), (long)rows) * rows;
        const long p0 = (long)xcd_block(blockIdx.x, gridDim.x) * ppb, p1 = min(npix, p0 + ppb);
        PixCursor cur;
        cur.init(p0 + r, d.H, d.W);
        uint2 xr[9], gr[4];
        auto fetch = [&](long p, uint2 (&xo)[9], uint2 (&go)[4]) {
            const bool in = p < p1;
            const unsigned base = in ? (unsigned)(p * n + c) : (unsigned)c;
            const unsigned mask = in ? tap_mask(cur.y, cur.x, dl, d.H, d.W) : 0u;
#pragma unroll
            for (int t = 0; t < 9; ++t) xo[t] = ld_tap8(x, base + (unsigned)toff[t], base, (mask >> t) & 1u);
            const unsigned gb = 4u * (base - (unsigned)c) + (unsigned)c;
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) go[bb] = ld_tap8(g, gb + (unsigned)(bb * n), gb, in);
            cur.advance(rows, d.H, d.W);
        };
        long p = p0 + r;
        fetch(p, xr, gr);
        for (; p < p1; p += rows) {
            uint2 xn[9], gn[4];
            fetch(p + rows, xn, gn);
            f32x2_t gs[4][2];           // suffix sums g_b = sum_{b' >= b} dy_b' (the HFF adds of the forward, eesp.py:96-101)
            bf16x4_unpack(gr[3], gs[3]);
#pragma unroll
            for (int bb = 2; bb >= 0; --bb) {
                f32x2_t tv[2];
                bf16x4_unpack(gr[bb], tv);
                gs[bb][0] = gs[bb + 1][0] + tv[0];
                gs[bb][1] = gs[bb + 1][1] + tv[1];
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                f32x2_t xv[2];
                bf16x4_unpack(xr[t], xv);
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) {
                    acc[(bb * 9 + t) * 2] = pk_fma(xv[0], gs[bb][0], acc[(bb * 9 + t) * 2]);
                    acc[(bb * 9 + t) * 2 + 1] = pk_fma(xv[1], gs[bb][1], acc[(bb * 9 + t) * 2 + 1]);
                }
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) xr[t] = xn[t];
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) gr[bb] = gn[bb];
        }
    }
    // lanes r * cvn + cv, cvn <= 16: the two wave halves and the two rows of a half always hold different pixels
#pragma unroll
    for (int j = 0; j < 36; ++j) swap_add32(acc[j], acc[j + 36]);
#pragma unroll
    for (int j = 0; j < 18; ++j) swap_add16(acc[j], acc[j + 18]);
    if (cvn <= 8) {
#pragma unroll
        for (int j = 0; j < 18; ++j) {
            acc[j].x = lane_step_sum(acc[j].x, 8);
            acc[j].y = lane_step_sum(acc[j].y, 8);
        }
    }
    if (cvn <= 4) {
#pragma unroll
        for (int j = 0; j < 18; ++j) {
            acc[j].x = lane_step_sum(acc[j].x, 4);
            acc[j].y = lane_step_sum(acc[j].y, 4);
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if ((lane & 15) < cvn) {
        // register j of this lane = float pair 2 j, 2 j + 1 of the 144 = [36 (branch, tap)][4 channels], offset by 36 floats
        // in the odd rows and by 72 in the upper half of the wave
        const int bt0 = 9 * ((lane >> 4) & 1) + 18 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < 18; ++j) {
            float* dst = s_red + (long)(wid * 36 + bt0 + j / 2) * n + c + 2 * (j % 2);
            dst[0] = acc[j].x;
            dst[1] = acc[j].y;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 36 * n; e += 256) {
        const float sum = (s_red[e] + s_red[36 * n + e]) + (s_red[72 * n + e] + s_red[108 * n + e]);
        if (part) part[(long)blockIdx.x * 36 * n + e] = sum;      // dw layout [4][3][3][n]
        else atomicAdd(d.dw + e, sum);
    }
}

// the vectorised weight gradients take d: LEDN_PYRBW_SAME, LEDN_PYRBW_BF16_FROM_DY or LEDN_PYRBW_BF16, grid and ending
bool pyr_bwd_weight_bf16_plan(const ledn_pyrbwd_desc& d, DwPlan* p) {   // used by backward.hip
    const int cvn = d.n / 8;
    if (d.dtype != LEDN_BF16 || d.n % 8 || !pow2(cvn) || cvn > 64 || (long)d.N * d.H * d.W * d.n * 4 >= (1L << 31))
        return false;
    const int rows = 256 / cvn;
    static const bool same_on = exp_knob("LEDN_PYR_WGRAD_SAME", 1) != 0;     // (A/B knob)
    if (same_on && pyr_tile_applies(d) && d.n <= 64 && d.dil[1] == d.dil[0] && d.dil[2] == d.dil[0] && d.dil[3] == d.dil[0]) {
        const int rows4 = 256 / (d.n / 4);
        long nb4 = cdiv((long)d.N * d.H * d.W, rows4 * 4);
        if (nb4 > 512) nb4 = 512;            // one resident round: two workgroups per CU by the registers
        float* part4 = (nb4 > 32 || det()) ? ws_take(nb4 * 36 * d.n) : nullptr;
        if (!part4 && nb4 > 128) nb4 = 128;
        p->kid = LEDN_PYRBW_SAME;
        p->nb = p->rows = nb4;
        p->part = part4;
        return true;
    }
    long nb = cdiv((long)d.N * d.Ho * d.Wo, rows * 8);
    if (nb > 512) nb = 512;
    float* part = (nb > 32 || det()) ? ws_take(nb * 36 * d.n) : nullptr;
    if (!part && nb > 128) nb = 128;
    p->kid = pyr_from_dy(d) ? LEDN_PYRBW_BF16_FROM_DY : LEDN_PYRBW_BF16;
    p->nb = p->rows = nb;
    p->part = part;
    return true;
}

int pyr_bwd_weight_bf16(const ledn_pyrbwd_desc& d, const DwPlan& p, hipStream_t s) {   // used by backward.hip
    if (p.kid == LEDN_PYRBW_SAME)
        LEDN_LAUNCH(pyr_bwd_weight_same_kernel, dim3((unsigned)p.nb), dim3(256), (size_t)(144 * d.n) * sizeof(float), s, d,
                    p.part);
    else
        LEDN_LAUNCH(pyr_bwd_weight_bf16_kernel, dim3((unsigned)p.nb, 4u), dim3(256), (size_t)(36 * d.n) * sizeof(float), s, d,
                    p.part, p.kid == LEDN_PYRBW_BF16_FROM_DY);
    if (p.part) return finish_partials(p.part, (int)p.rows, 36 * d.n, 1, d.dw, nullptr, nullptr, s);
    return check_launch();
}

}  // namespace ledn
