// head_mc.hip -- LEDHead's head_x1 / head_x2 for more than two classes: norm -> act -> conv3x3 (pad 1, stride 1, 32 -> Co),
// 3 <= Co <= 32, bf16, on the matrix cores.  Three wave-autonomous kernels in the style of conv3x3.hip's narrow kernels:
//
//   head_mc_fwd_kernel    z[p][o]  = sum_{tap, c} t[p + off(tap)][c] w[o][c][tap],  t = act(x * scale + shift) (zero outside
//                         the image AFTER the prologue), epilogue v = z * out_scale + out_shift, optional ReLU, bf16 | f32
//   head_mc_dgrad_kernel  dy[p][c] = sum_{tap, o} dz[p - off(tap)][o] w[o][c][tap]   (ledn_conv2d, transposed = 1), bf16
//   head_mc_wgrad_kernel  dw[o][c][tap] += sum_p dz[p][o] t[p + off(tap)][c]          (ledn_conv2d_wgrad), f32 partial rows
//
// Tile mapping.  A wave owns a strip of 32 pixel columns and walks down a segment of rows; the three input rows of the
// strip (34 pixels: one halo column each side) live in a wave-private LDS ring [pixel][32 channels] (80-byte pixel stride),
// so the nine taps are address offsets.  The class axis is padded to ONE 32-wide matrix tile in registers / LDS only:
//   forward:  v_mfma_f32_32x32x16_bf16, A = w[o (padded to 32)][16 c], B = t[16 c][32 pixels] (one 16-byte LDS read per lane,
//             tap and K-step), 9 x 2 instructions per 32 pixels; D = [class][pixel].
//   dgrad:    the same with dz in the ring (classes Co .. 31 of a ring pixel stay zero) and A = w[c][o (padded)], flipped taps;
//             the second K-step is skipped for Co <= 16.
//   wgrad:    v_mfma_f32_16x16x32_bf16, K = pixels: A = t^T and B = dz^T both through ds_read_b64_tr_b16 from the ring and
//             from a [32 pixels][32 classes] LDS tile; 9 taps x 2 channel tiles x (1 | 2) class tiles of accumulators live for
//             the whole wave; the four waves meet in LDS in a fixed order, one partial row [Co * 288] per workgroup,
//             finish_partials adds the rows into dw (ordered in deterministic mode).
//
// Alignment of the class axis.  A pixel's class vector is 2 Co bytes: with an odd Co (38 bytes at 19 classes) odd pixels are
// only 2-byte aligned, and so is the start of a strip row, ((n H + r) W + x0) Co elements from the base.  No access to a
// [.., Co] bf16 tensor assumes more than that: a strip row is one CONTIGUOUS run of elements; the run is covered by the
// 4-byte words of the tensor (the base pointer is 4-byte aligned: the gate checks it), word k of the run holding elements
// 2 k - p and 2 k - p + 1 with p = the parity of the run's first element index.  A word is loaded / stored as a dword only
// when BOTH halves lie inside the run; a half-covered first or last word becomes one 2-byte access.  So every dword access
// is 4-byte aligned and nothing outside the run -- hence nothing outside the tensor -- is touched.  Between the run and
// the [pixel][class] LDS image elements move as 2-byte LDS accesses (element e -> pixel e / Co, class e % Co by a
// multiply-shift that is exact for e < 2048).  f32 logits are 4-byte elements: always aligned.  The 32-channel tensors
// (x, dy) are 64 bytes per pixel: 16-byte pieces as in the two-class kernels (the gate checks the base pointers).
#include "regconv.h"

namespace ledn {

constexpr int MC_C = 32;        // input channels of the heads (the backbone's `channels`)
constexpr int MC_PW = 34;       // pixels of a ring row: x0 - 1 .. x0 + 32
constexpr int MC_PIXB = 80;     // LDS bytes per pixel (64 + 16: 16-byte reads of neighbouring pixels on different banks)
constexpr int MC_ROWB = MC_PW * MC_PIXB;

struct McArgs {
    const bf16_t* x;            // forward / wgrad: the heads' input [N,H,W,32]
    const bf16_t* z;            // dgrad / wgrad: dz [N,H,W,Co]
    const float* w;             // OIHW f32 [Co][32][3][3]
    void* y;                    // forward: z (bf16 | f32) [N,H,W,Co]; dgrad: dy bf16 [N,H,W,32]
    float* part;                // wgrad: [gridDim.x][Co * 288]
    const float *in_scale, *in_shift, *in_slope, *out_scale, *out_shift;
    int in_act, act_out;
    int N, H, W, Co;
    int strips, segs, RS;
    long tasks;
};

// ---- the x ring: 16-byte pieces, prologue applied while writing, zero outside the image ---------------------------------
struct McPro {
    float sc[8], sh[8], ng[8];  // channels 8 (lane & 3) + i
};
__device__ __forceinline__ McPro mc_pro(const McArgs& a, int lane) {
    McPro p;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = 8 * (lane & 3) + i;
        p.sc[i] = a.in_scale ? a.in_scale[c] : 1.f;
        p.sh[i] = a.in_shift ? a.in_shift[c] : 0.f;
        p.ng[i] = a.in_act == LEDN_ACT_PRELU ? a.in_slope[c] : (a.in_act == LEDN_ACT_NONE ? 1.f : 0.f);
    }
    return p;
}
// piece e = lane + 64 t of a ring row: pixel e >> 2, channel octet e & 3 = lane & 3
__device__ __forceinline__ void mc_fetch_x(const bf16_t* xn, int ir, int x0, int H, int W, int lane, uint4 (&rw)[3]) {
    const bool rok = ir >= 0 && ir < H;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int e = lane + 64 * t, px = x0 - 1 + (e >> 2);
        const bool ok = rok && e < MC_PW * 4 && px >= 0 && px < W;
        uint4 v = *reinterpret_cast<const uint4*>(xn + (ok ? ((long)ir * W + px) * MC_C + 8 * (lane & 3) : 0L));
        if (!ok) v = make_uint4(0u, 0u, 0u, 0u);
        rw[t] = v;
    }
}
__device__ __forceinline__ void mc_commit_x(unsigned char* row, int ir, int x0, int H, int W, int lane, const uint4 (&rw)[3],
                                            const McPro& p) {
    const bool rok = ir >= 0 && ir < H;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int e = lane + 64 * t, px = x0 - 1 + (e >> 2);
        if (e >= MC_PW * 4) continue;
        const bool ok = rok && px >= 0 && px < W;
        uint4 v = __builtin_bit_cast(uint4, c11_prologue(__builtin_bit_cast(bf16x8_t, rw[t]), p.sc, p.sh, p.ng));
        if (!ok) v = make_uint4(0u, 0u, 0u, 0u);                         // padding is zero AFTER the activation
        *reinterpret_cast<uint4*>(row + (e >> 2) * MC_PIXB + (lane & 3) * 16) = v;
    }
}

// ---- a run of [pixels][Co] bf16 elements <-> the [pixel][class] LDS image (see "Alignment" in the header) ----------------
struct McRun {
    long g0;                    // element index of the run's first element from the tensor base
    int nel, par, poff;         // elements, parity of g0, LDS pixel of the run's first pixel
};
__device__ __forceinline__ McRun mc_run(int img, int ir, int pxa, int pxb, int px_lds0, int H, int W, int Co, bool rok) {
    McRun r;
    r.g0 = (((long)img * H + (rok ? ir : 0)) * W + pxa) * Co;
    r.nel = rok && pxb > pxa ? (pxb - pxa) * Co : 0;
    r.par = (int)(r.g0 & 1);
    r.poff = pxa - px_lds0;
    return r;
}
template <int ND>
__device__ __forceinline__ void mc_fetch_run(const bf16_t* z, const McRun& r, int lane, unsigned (&rz)[ND]) {
#pragma unroll
    for (int t = 0; t < ND; ++t) {
        const int e0 = 2 * (lane + 64 * t) - r.par, e1 = e0 + 1;
        const bool ok0 = e0 >= 0 && e0 < r.nel, ok1 = e1 < r.nel;
        unsigned v = 0u;
        if (ok0 && ok1) v = *reinterpret_cast<const unsigned*>(z + r.g0 + e0);      // (g0 + e0 even: 4-byte aligned)
        else if (ok0) v = (unsigned)z[r.g0 + e0].v;
        else if (ok1) v = (unsigned)z[r.g0 + e1].v << 16;
        rz[t] = v;
    }
}
// pixels of the LDS row outside [lo, hi) (image border, rows outside the image): all 32 classes zero
__device__ __forceinline__ void mc_zero_px(unsigned char* row, int lane, int npx, int lo, int hi) {
    if (lane < npx && (lane < lo || lane >= hi)) {
        uint4* p = reinterpret_cast<uint4*>(row + lane * MC_PIXB);
        p[0] = p[1] = p[2] = p[3] = make_uint4(0u, 0u, 0u, 0u);
    }
}
template <int ND>
__device__ __forceinline__ void mc_commit_run(unsigned char* row, const McRun& r, int Co, unsigned rcp, int lane,
                                              const unsigned (&rz)[ND]) {
#pragma unroll
    for (int t = 0; t < ND; ++t) {
        const int e0 = 2 * (lane + 64 * t) - r.par, e1 = e0 + 1;
        if (e0 >= 0 && e0 < r.nel) {
            const int q = (int)(((unsigned)e0 * rcp) >> 16);
            *reinterpret_cast<unsigned short*>(row + (r.poff + q) * MC_PIXB + (e0 - q * Co) * 2) = (unsigned short)(rz[t] & 0xffffu);
        }
        if (e1 < r.nel) {
            const int q = (int)(((unsigned)e1 * rcp) >> 16);
            *reinterpret_cast<unsigned short*>(row + (r.poff + q) * MC_PIXB + (e1 - q * Co) * 2) = (unsigned short)(rz[t] >> 16);
        }
    }
}

struct McTask {
    int img, x0, r0, r1;
};
__device__ __forceinline__ McTask mc_task(const McArgs& a, long task) {
    McTask t;
    const int strip = (int)(task % a.strips), seg = (int)((task / a.strips) % a.segs);
    t.img = (int)(task / ((long)a.strips * a.segs));
    t.x0 = strip * 32;
    t.r0 = seg * a.RS;
    t.r1 = min(t.r0 + a.RS, a.H);
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
template <bool OUT16>
__global__ void __launch_bounds__(256, 2) head_mc_fwd_kernel(McArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_x[4][3 * MC_ROWB];
    __shared__ __attribute__((aligned(16))) float s_o[4][32 * 32];                // [pixel][Co] of one output row (f32 | bf16)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, n = lane & 31, h = lane >> 5;
    const int H = a.H, W = a.W, Co = a.Co;
    unsigned char* ring = &s_x[wid][0];
    // A[m = class][k = channel 16 s + 8 h + j] of tap t; classes Co .. 31 are zero rows
    bf16x8_t af[9][2];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 16 * s + 8 * h + j;
                af[t][s][j] = (short)(n < Co ? f32_to_bf16(a.w[(n * MC_C + c) * 9 + t]) : (unsigned short)0);
            }
    const McPro pro = mc_pro(a, lane);
    // epilogue coefficients of this lane's 16 classes (D row of register reg)
    float osc[16], osh[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int co = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        osc[reg] = (a.out_scale && co < Co) ? a.out_scale[co] : 1.f;
        osh[reg] = (a.out_shift && co < Co) ? a.out_shift[co] : 0.f;
    }
    const bool relu = a.act_out == LEDN_ACT_RELU;
    float* so = s_o[wid];
    const long nwaves = (long)gridDim.x * 4;
    for (long task = (long)blockIdx.x * 4 + wid; task < a.tasks; task += nwaves) {
        const McTask tk = mc_task(a, task);
        const int x0 = tk.x0, r0 = tk.r0, r1 = tk.r1;
        const bf16_t* xn = a.x + (long)tk.img * H * W * MC_C;
        const int nvalid = min(32, W - x0), nel = nvalid * Co;
        uint4 xr[3];
        mc_fetch_x(xn, r0 - 1, x0, H, W, lane, xr);
        mc_commit_x(ring, r0 - 1, x0, H, W, lane, xr, pro);
        mc_fetch_x(xn, r0, x0, H, W, lane, xr);
        mc_commit_x(ring + MC_ROWB, r0, x0, H, W, lane, xr, pro);
        mc_fetch_x(xn, r0 + 1, x0, H, W, lane, xr);                      // committed in the first iteration
        int slot_new = 2;                                                // slot the row o + 1 goes to
        for (int o = r0; o < r1; ++o) {
            wave_sync();                                                 // the previous row's reads of slot_new and of so are done
            mc_commit_x(ring + slot_new * MC_ROWB, o + 1, x0, H, W, lane, xr, pro);
            if (o + 1 < r1) mc_fetch_x(xn, o + 2, x0, H, W, lane, xr);
            wave_sync();
            const int s_top = slot_new == 2 ? 0 : slot_new + 1;          // slot of row o - 1
            f32x16_t acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                int sl = s_top + kh;
                sl = sl >= 3 ? sl - 3 : sl;
                const unsigned char* row = ring + sl * MC_ROWB + n * MC_PIXB + 16 * h;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const uint4 b = *reinterpret_cast<const uint4*>(row + kw * MC_PIXB + 32 * s);
                        acc = mfma_32x32x16_bf16(af[kh * 3 + kw][s], __builtin_bit_cast(bf16x8_t, b), acc);
                    }
            }
            // D[class = (reg & 3) + 8 (reg >> 2) + 4 h][pixel n] -> so[pixel][class]
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int co = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                float v = fmaf(acc[reg], osc[reg], osh[reg]);
                if (relu) v = fmaxf(v, 0.f);
                if (co < Co) {
                    if (OUT16) reinterpret_cast<unsigned short*>(so)[n * Co + co] = f32_to_bf16(v);
                    else so[n * Co + co] = v;
                }
            }
            wave_sync();
            // the row's nvalid * Co elements are one contiguous run of the output
            const long g0 = (((long)tk.img * H + o) * W + x0) * Co;
            if (OUT16) {
                bf16_t* y = reinterpret_cast<bf16_t*>(a.y);
                const unsigned short* s16 = reinterpret_cast<const unsigned short*>(so);
                const int par = (int)(g0 & 1), ndw = (par + nel + 1) >> 1;
                for (int k = lane; k < ndw; k += 64) {
                    const int e0 = 2 * k - par, e1 = e0 + 1;
                    const bool ok0 = e0 >= 0, ok1 = e1 < nel;
                    if (ok0 && ok1) *reinterpret_cast<unsigned*>(y + g0 + e0) = (unsigned)s16[e0] | ((unsigned)s16[e1] << 16);
                    else if (ok0) y[g0 + e0].v = s16[e0];
                    else if (ok1) y[g0 + e1].v = s16[e1];
                }
            } else {
                float* y = reinterpret_cast<float*>(a.y);
                for (int e = lane; e < nel; e += 64) y[g0 + e] = so[e];
            }
            slot_new = slot_new == 2 ? 0 : slot_new + 1;
        }
        wave_sync();                                                     // the next task rewrites the ring
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// data gradient
// ---------------------------------------------------------------------------------------------------------------------
template <int NS>       // K-steps over the padded class axis: 1 for Co <= 16
__global__ void __launch_bounds__(256, 2) head_mc_dgrad_kernel(McArgs a) {
    constexpr int ND = NS == 1 ? 5 : 9;                                  // dwords per lane of a 34-pixel run: (34 * 16 | 32 + 2) / 2 / 64
    __shared__ __attribute__((aligned(16))) unsigned char s_z[4][3 * MC_ROWB];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, n = lane & 31, h = lane >> 5;
    const int H = a.H, W = a.W, Co = a.Co;
    const unsigned rcp = 65536u / (unsigned)Co + 1u;
    unsigned char* ring = &s_z[wid][0];
    for (int i = lane; i < 3 * MC_ROWB / 16; i += 64) reinterpret_cast<uint4*>(ring)[i] = make_uint4(0u, 0u, 0u, 0u);
    wave_sync();
    // A[m = input channel c][k = class 16 s + 8 h + j] of ring tap t = the filter's tap 8 - t
    bf16x8_t af[9][NS];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int o = 16 * s + 8 * h + j;
                af[t][s][j] = (short)(o < Co ? f32_to_bf16(a.w[((o < Co ? o : 0) * MC_C + n) * 9 + (8 - t)]) : (unsigned short)0);
            }
    bf16_t* y = reinterpret_cast<bf16_t*>(a.y);
    const long nwaves = (long)gridDim.x * 4;
    for (long task = (long)blockIdx.x * 4 + wid; task < a.tasks; task += nwaves) {
        const McTask tk = mc_task(a, task);
        const int x0 = tk.x0, r0 = tk.r0, r1 = tk.r1;
        const int pxa = max(x0 - 1, 0), pxb = min(x0 + 33, W);
        auto run_of = [&](int ir) { return mc_run(tk.img, ir, pxa, pxb, x0 - 1, H, W, Co, ir >= 0 && ir < H); };
        auto commit = [&](int ir, int slot, const unsigned (&rz)[ND]) {
            const McRun r = run_of(ir);
            unsigned char* row = ring + slot * MC_ROWB;
            const bool rok = ir >= 0 && ir < H;
            mc_zero_px(row, lane, MC_PW, rok ? pxa - (x0 - 1) : MC_PW, rok ? pxb - (x0 - 1) : 0);
            mc_commit_run<ND>(row, r, Co, rcp, lane, rz);
        };
        unsigned zr[ND];
        mc_fetch_run<ND>(a.z, run_of(r0 - 1), lane, zr);
        commit(r0 - 1, 0, zr);
        mc_fetch_run<ND>(a.z, run_of(r0), lane, zr);
        commit(r0, 1, zr);
        mc_fetch_run<ND>(a.z, run_of(r0 + 1), lane, zr);
        int slot_new = 2;
        for (int o = r0; o < r1; ++o) {
            wave_sync();
            commit(o + 1, slot_new, zr);
            if (o + 1 < r1) mc_fetch_run<ND>(a.z, run_of(o + 2), lane, zr);
            wave_sync();
            const int s_top = slot_new == 2 ? 0 : slot_new + 1;
            f32x16_t acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                int sl = s_top + kh;
                sl = sl >= 3 ? sl - 3 : sl;
                const unsigned char* row = ring + sl * MC_ROWB + n * MC_PIXB + 16 * h;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const uint4 b = *reinterpret_cast<const uint4*>(row + kw * MC_PIXB + 32 * s);
                        acc = mfma_32x32x16_bf16(af[kh * 3 + kw][s], __builtin_bit_cast(bf16x8_t, b), acc);
                    }
            }
            // D[channel = (reg & 3) + 8 (reg >> 2) + 4 h][pixel n]: four 8-byte pieces of the pixel's 64 bytes
            if (x0 + n < W) {
                bf16_t* yp = y + ((((long)tk.img * H + o) * W + x0 + n) * MC_C + 4 * h);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float v[4] = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                    st4(yp + 8 * g, v);
                }
            }
            slot_new = slot_new == 2 ? 0 : slot_new + 1;
        }
        wave_sync();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MC_ZTB = 32 * MC_PIXB;                                     // the dz tile of a wave: [32 pixels][32 classes]
template <int NT>       // 16-class tiles: 1 for Co <= 16
__global__ void __launch_bounds__(256, 2) head_mc_wgrad_kernel(McArgs a) {
    constexpr int ND = NT == 1 ? 5 : 9;                                  // (32 * 16 | 32 + 2) / 2 / 64 dwords per lane
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[4 * (3 * MC_ROWB + MC_ZTB)];    // 42 880 B >= the 32 x 288 f32 of the reduction
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, m16 = lane & 15, q = lane >> 4;
    const int H = a.H, W = a.W, Co = a.Co;
    const unsigned rcp = 65536u / (unsigned)Co + 1u;
    unsigned char* ring = s_raw + wid * (3 * MC_ROWB + MC_ZTB);
    unsigned char* zt = ring + 3 * MC_ROWB;
    for (int i = lane; i < MC_ZTB / 16; i += 64) reinterpret_cast<uint4*>(zt)[i] = make_uint4(0u, 0u, 0u, 0u);
    wave_sync();
    const McPro pro = mc_pro(a, lane);
    f32x4_t acc[9][2][NT];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[t][mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const long nwaves = (long)gridDim.x * 4;
    for (long task = (long)blockIdx.x * 4 + wid; task < a.tasks; task += nwaves) {
        const McTask tk = mc_task(a, task);
        const int x0 = tk.x0, r0 = tk.r0, r1 = tk.r1;
        const bf16_t* xn = a.x + (long)tk.img * H * W * MC_C;
        const int pxb = min(x0 + 32, W);
        auto run_of = [&](int ir) { return mc_run(tk.img, ir, x0, pxb, x0, H, W, Co, ir < r1); };
        uint4 xr[3];
        unsigned zr[ND];
        mc_fetch_x(xn, r0 - 1, x0, H, W, lane, xr);
        mc_commit_x(ring, r0 - 1, x0, H, W, lane, xr, pro);
        mc_fetch_x(xn, r0, x0, H, W, lane, xr);
        mc_commit_x(ring + MC_ROWB, r0, x0, H, W, lane, xr, pro);
        mc_fetch_x(xn, r0 + 1, x0, H, W, lane, xr);
        mc_fetch_run<ND>(a.z, run_of(r0), lane, zr);
        mc_zero_px(zt, lane, 32, 0, pxb - x0);                           // (the strip's width is the same for all its rows)
        int slot_new = 2;
        for (int o = r0; o < r1; ++o) {
            wave_sync();                                                 // the previous iteration's reads of slot_new and zt are done
            mc_commit_x(ring + slot_new * MC_ROWB, o + 1, x0, H, W, lane, xr, pro);
            mc_commit_run<ND>(zt, run_of(o), Co, rcp, lane, zr);
            if (o + 1 < r1) {
                mc_fetch_x(xn, o + 2, x0, H, W, lane, xr);
                mc_fetch_run<ND>(a.z, run_of(o + 1), lane, zr);
            }
            wave_sync();
            // B[k = pixel 8 q + j][n = class 16 nt + m16]: lane 4 r + p supplies pixel 8 q + r (+ 4), classes 16 nt + 4 p ..
            bf16x8_t bz[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const unsigned char* bp = zt + (8 * q + (m16 >> 2)) * MC_PIXB + (16 * nt + 4 * (m16 & 3)) * 2;
                const bf16x4_t lo = lds_read_tr16(bp), hi4 = lds_read_tr16(bp + 4 * MC_PIXB);
                bz[nt][0] = lo[0]; bz[nt][1] = lo[1]; bz[nt][2] = lo[2]; bz[nt][3] = lo[3];
                bz[nt][4] = hi4[0]; bz[nt][5] = hi4[1]; bz[nt][6] = hi4[2]; bz[nt][7] = hi4[3];
            }
            const int s_top = slot_new == 2 ? 0 : slot_new + 1;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                int sl = s_top + kh;
                sl = sl >= 3 ? sl - 3 : sl;
                const unsigned char* row = ring + sl * MC_ROWB;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        // ring pixel of (output pixel x0 + 8 q + j, tap kw) = 8 q + j + kw
                        const unsigned char* ap = row + (8 * q + kw + (m16 >> 2)) * MC_PIXB + (16 * mt + 4 * (m16 & 3)) * 2;
                        const bf16x4_t lo = lds_read_tr16(ap), hi4 = lds_read_tr16(ap + 4 * MC_PIXB);
                        bf16x8_t af;
                        af[0] = lo[0]; af[1] = lo[1]; af[2] = lo[2]; af[3] = lo[3];
                        af[4] = hi4[0]; af[5] = hi4[1]; af[6] = hi4[2]; af[7] = hi4[3];
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[kh * 3 + kw][mt][nt] = mfma_16x16x32_bf16(af, bz[nt], acc[kh * 3 + kw][mt][nt]);
                    }
            }
            slot_new = slot_new == 2 ? 0 : slot_new + 1;
        }
        wave_sync();
    }
    // acc[t][mt][nt][i] = dW[class 16 nt + m16][channel 16 mt + 4 q + i][tap t]: the four waves add up in LDS in wave order
    float* s_red = reinterpret_cast<float*>(s_raw);
    for (int wv = 0; wv < 4; ++wv) {
        __syncthreads();
        if (wid == wv) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int co = 16 * nt + m16;
                if (co < Co) {
#pragma unroll
                    for (int t = 0; t < 9; ++t)
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                float* p = s_red + co * 288 + (16 * mt + 4 * q + i) * 9 + t;
                                *p = wv ? *p + acc[t][mt][nt][i] : acc[t][mt][nt][i];
                            }
                }
            }
        }
    }
    __syncthreads();
    const int nel = Co * 288;
    for (int e = tid; e < nel; e += 256) a.part[(long)blockIdx.x * nel + e] = s_red[e];
}

// ---------------------------------------------------------------------------------------------------------------------
// gates and launchers
// ---------------------------------------------------------------------------------------------------------------------
static bool mc_on() {
    static const bool on = exp_knob("LEDN_HEAD_MC", 1) != 0;             // (A/B knob: 0 = the generic kernels)
    return on && (options().stream_fast & 64) != 0;
}
static bool mc_aligned(const void* p, unsigned n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
static bool mc_shape(int N, int H, int W, int Ho, int Wo, int KH, int KW, int stride, int pad, int dil, int groups) {
    if (KH != 3 || KW != 3 || stride != 1 || pad != 1 || dil != 1 || groups != 1 || Ho != H || Wo != W) return false;
    const long npix = (long)N * H * W;
    return N >= 1 && H >= 1 && W >= 1 && npix >= 1024 && npix * MC_C < (1L << 31);
}

// 0: not ours; 1: the heads' forward (prologue present: the norm -> act in front of the convolution); 2: their data gradient
// (no packed weights: a caller that supplies ledn_pack_conv_weights' pack asks for the general matrix-core kernels)
int head_mc_conv_kind(const ledn_conv_desc& d) {
    if (!mc_on() || d.dtype_x != LEDN_BF16 || !d.w || !d.x || !d.y) return 0;
    if (!mc_shape(d.N, d.H, d.W, d.Ho, d.Wo, d.KH, d.KW, d.stride, d.pad, d.dil, d.groups)) return 0;
    if (d.xadd || d.res || d.res_mode != LEDN_RES_NONE || d.stat_sum || d.stat_sqsum) return 0;
    if (!d.transposed) {
        if (d.Cin != MC_C || d.Cout < 3 || d.Cout > 32) return 0;
        if (d.dtype_y != LEDN_BF16 && d.dtype_y != LEDN_F32) return 0;
        if (!d.in_scale || !d.in_shift) return 0;
        if (d.in_act != LEDN_ACT_NONE && d.in_act != LEDN_ACT_RELU && !(d.in_act == LEDN_ACT_PRELU && d.in_slope)) return 0;
        if (d.act_out != LEDN_ACT_NONE && d.act_out != LEDN_ACT_RELU) return 0;
        if (d.ws_co != (long long)MC_C * 9 || d.ws_ci != 9 || d.ws_tap != 1) return 0;
        if (!mc_aligned(d.x, 16) || !mc_aligned(d.y, 4)) return 0;
        return 1;
    }
    if (d.Cout != MC_C || d.Cin < 3 || d.Cin > 32 || d.dtype_y != LEDN_BF16 || d.w_bf16) return 0;
    if (d.in_scale || d.in_shift || d.in_act != LEDN_ACT_NONE || d.out_scale || d.out_shift || d.act_out != LEDN_ACT_NONE) return 0;
    if (d.ws_co != 9 || d.ws_ci != (long long)MC_C * 9 || d.ws_tap != 1) return 0;      // OIHW seen from the gradient's side
    if (!mc_aligned(d.x, 4) || !mc_aligned(d.y, 16)) return 0;
    return 2;
}

bool head_mc_wgrad_supported(const ledn_wgrad_desc& d) {
    if (!mc_on() || d.dtype_x != LEDN_BF16 || d.dtype_dz != LEDN_BF16 || d.xadd || !d.x || !d.dz || !d.dw) return false;
    if (!mc_shape(d.N, d.H, d.W, d.Ho, d.Wo, d.KH, d.KW, d.stride, d.pad, d.dil, d.groups)) return false;
    if (d.Cin != MC_C || d.Cout < 3 || d.Cout > 32 || !d.in_scale || !d.in_shift) return false;
    if (d.in_act != LEDN_ACT_NONE && d.in_act != LEDN_ACT_RELU && !(d.in_act == LEDN_ACT_PRELU && d.in_slope)) return false;
    if (d.ws_co != (long long)MC_C * 9 || d.ws_ci != 9 || d.ws_tap != 1) return false;   // the partial rows use dW's own index
    return mc_aligned(d.x, 16) && mc_aligned(d.dz, 4);
}

// rows per task: the longest of 32 / 16 / 8 that still yields two tasks per resident wave (a task re-reads 2 halo rows)
static void mc_tasks(McArgs& a) {
    a.strips = (int)cdiv(a.W, 32);
    const long columns = (long)a.N * a.strips;
    a.RS = columns * cdiv(a.H, 32) >= 4096 ? 32 : (columns * cdiv(a.H, 16) >= 2048 ? 16 : 8);
    a.segs = (int)cdiv(a.H, a.RS);
    a.tasks = columns * a.segs;
}
static long mc_blocks(const McArgs& a) {
    const long nb = cdiv(a.tasks, 4L), cap = (long)options().conv_workgroups * 2;
    return nb > cap ? cap : nb;
}

int head_mc_conv(const ledn_conv_desc& d, hipStream_t s) {
    const int kind = head_mc_conv_kind(d);
    LEDN_REQUIRE(kind != 0);
    McArgs a = {};
    a.w = d.w; a.y = d.y;
    a.N = d.N; a.H = d.H; a.W = d.W;
    mc_tasks(a);
    const unsigned nb = (unsigned)mc_blocks(a);
    if (kind == 1) {
        a.x = (const bf16_t*)d.x; a.Co = d.Cout;
        a.in_scale = d.in_scale; a.in_shift = d.in_shift; a.in_slope = d.in_slope; a.in_act = d.in_act;
        a.out_scale = d.out_scale; a.out_shift = d.out_shift; a.act_out = d.act_out;
        if (d.dtype_y == LEDN_BF16) LEDN_LAUNCH((head_mc_fwd_kernel<true>), dim3(nb), dim3(256), 0, s, a);
        else LEDN_LAUNCH((head_mc_fwd_kernel<false>), dim3(nb), dim3(256), 0, s, a);
    } else {
        a.z = (const bf16_t*)d.x; a.Co = d.Cin;
        if (a.Co <= 16) LEDN_LAUNCH((head_mc_dgrad_kernel<1>), dim3(nb), dim3(256), 0, s, a);
        else LEDN_LAUNCH((head_mc_dgrad_kernel<2>), dim3(nb), dim3(256), 0, s, a);
    }
    return check_launch();
}

// needs the bound workspace for its partial rows (LEDN_EINVAL without one, as conv_wgrad_narrow_reg)
int head_mc_wgrad(const ledn_wgrad_desc& d, hipStream_t s) {
    LEDN_REQUIRE(head_mc_wgrad_supported(d));
    McArgs a = {};
    a.x = (const bf16_t*)d.x; a.z = (const bf16_t*)d.dz;
    a.in_scale = d.in_scale; a.in_shift = d.in_shift; a.in_slope = d.in_slope; a.in_act = d.in_act;
    a.N = d.N; a.H = d.H; a.W = d.W; a.Co = d.Cout;
    mc_tasks(a);
    long nb = mc_blocks(a);
    const int nel = d.Cout * 288;
    const long room = workspace().ptr ? workspace().nfloats / nel : 0;
    if (nb > room) nb = room;
    if (nb < 1) return LEDN_EINVAL;
    a.part = ws_take(nb * nel);
    if (!a.part) return LEDN_EINVAL;
    if (a.Co <= 16) LEDN_LAUNCH((head_mc_wgrad_kernel<1>), dim3((unsigned)nb), dim3(256), 0, s, a);
    else LEDN_LAUNCH((head_mc_wgrad_kernel<2>), dim3((unsigned)nb), dim3(256), 0, s, a);
    return finish_partials(a.part, (int)nb, nel, 1, d.dw, nullptr, nullptr, s);
}

}  // namespace ledn
