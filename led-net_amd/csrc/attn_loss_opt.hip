// attn_loss_opt.hip -- window-attention backward, fused OHEM cross-entropy
// (radix-select threshold instead of the reference's full sort), multi-tensor SGD.
#include "ledn_rt.h"

namespace ledn {

// ===========================================================================
// Window attention backward.  One wavefront per (window, head); lane = token.
// Phase A (lane = query i): recompute P[i][:], dP = dO.V^T, dS = P*(dP - rowsum(P*dP)),
//   dQ[i] = scale * dS[i][:] . K ; dS kept in LDS (64x64 f32) and added to dbiasT.
// Phase B (lane = key j): dK[j] = scale * dS[:][j]^T . Q,  dV[j] = P[:][j]^T . dO.
// LDS: K, V, Q, dO (4 x 64 x D f32) + dS + P (2 x 16 KiB) = 48 KiB at D = 16.
// ===========================================================================
// The wavefront walks several windows of its head; the 64x64 score-gradient rows live in LDS with a
// 65-float row stride (lane = row in phase A, lane = column in phase B: both conflict-free; the
// 64-float stride of the first version put all 64 lanes on one bank), and the relative-position
// bias gradient is summed over the wavefront's windows in LDS and leaves as ONE partial table per
// wavefront (the first version issued one global atomic per score and window: 1024 same-address
// atomics per table entry at 16 x 64 x 64).
template <typename T, int D, bool PADDED>
__global__ void __launch_bounds__(64) window_attn_bwd_kernel(const T* qkv, const float* biasT, const T* dout,
                                                             float* dqkv, float* dbiasT, int N, int H,
                                                             int W, int C, int heads, int hh, int ww,
                                                             float* part, float* pad_out) {
    // LDS per wavefront: K, V, Q, dO (16 KB at D = 16) + ONE 64 x 65 score matrix that holds P and is then
    // overwritten by dS (dV = P^T dO is taken in between), the bias-gradient rows live in registers:
    // 33 KB -> four wavefronts per CU (the first version kept P, dS and the bias rows in LDS: 66 KB, two
    // wavefronts per CU, two of the four SIMDs idle).
    constexpr int WS = 8, T2 = 64, TP = 65;
    __shared__ float s_k[T2 * D], s_v[T2 * D], s_q[T2 * D], s_do[T2 * D];
    __shared__ float s_p[T2 * TP];
    const int head = blockIdx.y;
    const int t = threadIdx.x;
    const int nwin = N * hh * ww;
    const float scale = rsqrtf((float)D);
    const float* b = biasT + (long)head * T2 * T2 + t;
    float db[T2];                                  // bias-gradient row of query t, summed over this wave's windows
#pragma unroll
    for (int k = 0; k < T2; ++k) db[k] = 0.f;
    for (int win = blockIdx.x; win < nwin; win += gridDim.x) {
        const int wx = win % ww, wy = (win / ww) % hh, n = win / (ww * hh);
        const int y = wy * WS + t / WS, x = wx * WS + t % WS;
        const bool inside = y < H && x < W;
        const int ys = y < H ? y : 2 * H - 2 - y;
        const int xs = x < W ? x : 2 * W - 2 - x;
        const long src = ((long)n * H + ys) * W + xs;
        const T* p = qkv + src * (3L * C) + head * D;
        float q[D], go[D];
        __syncthreads();     // the previous window's last phase is done with the LDS operands
#pragma unroll
        for (int j = 0; j < D; j += 4) {
            float kv[4], vv[4];
            ldv<4>(p + j, q + j);
            ldv<4>(p + C + j, kv);
            ldv<4>(p + 2 * C + j, vv);
            if (inside) ldv<4>(dout + src * C + head * D + j, go + j);
            else {
#pragma unroll
                for (int i = 0; i < 4; ++i) go[j + i] = 0.f;  // cropped outputs carry no gradient
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s_k[t * D + j + i] = kv[i];
                s_v[t * D + j + i] = vv[i];
                s_q[t * D + j + i] = q[j + i];
                s_do[t * D + j + i] = go[j + i];
            }
        }
        __syncthreads();
        // ---- A1 (lane = query t): P[t][:] = softmax(q.K^T * scale + bias)
        float m = -3.0e38f;
        for (int k0 = 0; k0 < T2; k0 += 8) {
            float bk[8];                             // eight bias loads in flight (a dependent global load per
#pragma unroll                                       // score made this loop latency-bound)
            for (int u = 0; u < 8; ++u) bk[u] = b[(k0 + u) * T2];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + u;
                float dot = 0.f;
#pragma unroll
                for (int j = 0; j < D; ++j) dot = fmaf(q[j], s_k[k * D + j], dot);
                const float sc = dot * scale + bk[u];
                s_p[t * TP + k] = sc;
                m = fmaxf(m, sc);
            }
        }
        float l = 0.f;
        for (int k = 0; k < T2; ++k) {
            const float e = __expf(s_p[t * TP + k] - m);
            s_p[t * TP + k] = e;
            l += e;
        }
        const float inv = 1.f / l;
        float rs = 0.f;  // sum_k P*dP
        for (int k = 0; k < T2; ++k) {
            const float pk = s_p[t * TP + k] * inv;
            float dp = 0.f;
#pragma unroll
            for (int j = 0; j < D; ++j) dp = fmaf(go[j], s_v[k * D + j], dp);
            s_p[t * TP + k] = pk;
            rs = fmaf(pk, dp, rs);
        }
        __syncthreads();
        // ---- B1 (lane = key t): dV[t] = P[:, t]^T . dO
        float dv[D];
#pragma unroll
        for (int j = 0; j < D; ++j) dv[j] = 0.f;
        for (int i = 0; i < T2; ++i) {
            const float pk = s_p[i * TP + t];
#pragma unroll
            for (int j = 0; j < D; ++j) dv[j] = fmaf(pk, s_do[i * D + j], dv[j]);
        }
        __syncthreads();
        // ---- A2 (lane = query t): dS = P * (dP - rs) overwrites P (dP recomputed: 16 FMAs), dQ, bias rows
        float dq[D];
#pragma unroll
        for (int j = 0; j < D; ++j) dq[j] = 0.f;
#pragma unroll
        for (int k = 0; k < T2; ++k) {
            float dp = 0.f;
#pragma unroll
            for (int j = 0; j < D; ++j) dp = fmaf(go[j], s_v[k * D + j], dp);
            const float ds = s_p[t * TP + k] * (dp - rs);
            s_p[t * TP + k] = ds;
            db[k] += ds;
#pragma unroll
            for (int j = 0; j < D; ++j) dq[j] = fmaf(ds, s_k[k * D + j], dq[j]);
        }
        __syncthreads();
        // ---- B2 (lane = key t): dK[t] = scale * dS[:, t]^T . Q
        float dk[D];
#pragma unroll
        for (int j = 0; j < D; ++j) dk[j] = 0.f;
        for (int i = 0; i < T2; ++i) {
            const float ds = s_p[i * TP + t];
#pragma unroll
            for (int j = 0; j < D; ++j) dk[j] = fmaf(ds, s_q[i * D + j], dk[j]);
        }
        float* o = dqkv + src * (3L * C) + head * D;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (PADDED && pad_out) {    // deterministic mode: every padded position is stored once, window_attn_fold_kernel
                float* po = pad_out + (((long)n * (hh * WS) + y) * (ww * WS) + x) * (3L * C) + head * D;   // adds the copies
                po[j] = dq[j] * scale;
                po[C + j] = dk[j] * scale;
                po[2 * C + j] = dv[j];
            } else if (PADDED) {
                atomicAdd(o + j, dq[j] * scale);
                atomicAdd(o + C + j, dk[j] * scale);
                atomicAdd(o + 2 * C + j, dv[j]);
            } else {
                o[j] = dq[j] * scale;
                o[C + j] = dk[j] * scale;
                o[2 * C + j] = dv[j];
            }
        }
    }
    // bias-gradient table of this wavefront: dbiasT[head][k][t] (t = query row = lane)
#pragma unroll
    for (int k = 0; k < T2; ++k) {
        const long idx = (long)head * T2 * T2 + k * T2 + t;
        if (part) part[(long)blockIdx.x * heads * T2 * T2 + idx] = db[k];
        else atomicAdd(dbiasT + idx, db[k]);
    }
}

// ---------------------------------------------------------------------------
// Matrix-core variant (bf16, head dim 16, no reflect padding): the five 64 x 64 x 16 products of a
// (window, head) as v_mfma_f32_32x32x16_bf16.  Everything score-shaped is kept TRANSPOSED,
// S^T[key j][query i], so that an accumulator lane owns ONE query (column) and its registers run over
// the keys: the softmax / row-sum reductions are in-lane plus one exchange with lane ^ 32, and the
// bias-gradient table dbiasT[head][j][i] accumulates in the same register layout across the
// wavefront's windows.  S^T = K Q^T and dP^T = V dO^T take their fragments straight from global
// memory (16 B per lane); dQ^T = K^T dS^T uses the accumulator registers as the B operand (the
// contraction index is permuted consistently on the A side); dV^T = dO^T P and dK^T = Q^T dS need
// the score matrix transposed, which goes through one 64 x 64 bf16 LDS tile.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) window_attn_bwd_mfma_kernel(const bf16_t* qkv, const float* biasT,
                                                                  const bf16_t* dout, float* dqkv, float* dbiasT,
                                                                  int N, int H, int W, int C, int heads, int hh,
                                                                  int ww, float* part) {
    constexpr int D = 16, T2 = 64, LP = 72;      // LDS row stride (bf16 elements): 64 + 8 pad
    __shared__ __attribute__((aligned(16))) unsigned short s_kt[D * LP], s_qt[D * LP], s_dot[D * LP];
    __shared__ __attribute__((aligned(16))) unsigned short s_m[T2 * LP];
    const int head = blockIdx.y;
    const int lane = threadIdx.x, lr = lane & 31, lh = lane >> 5;
    const int nwin = N * hh * ww;
    const float scale = rsqrtf((float)D);
    // bias and its gradient in accumulator layout: [jt][it][reg] <-> key jt*32 + row(reg, lh), query it*32 + lr
    float bias[2][2][16], db[2][2][16];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, i = it * 32 + lr;
                bias[jt][it][r] = biasT[(long)head * T2 * T2 + j * T2 + i];
                db[jt][it][r] = 0.f;
            }
    const bf16x8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int win = blockIdx.x; win < nwin; win += gridDim.x) {
        const int wx = win % ww, wy = (win / ww) % hh, n = win / (ww * hh);
        // fragments of tokens lr and 32 + lr (rows of the two 32-row tiles), dims lh*8 .. lh*8+7
        bf16x8_t kf[2], vf[2], qf[2], dof[2];
        long tokoff[2];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            const int tok = tl * 32 + lr;
            const long pix = ((long)n * H + wy * 8 + tok / 8) * W + wx * 8 + tok % 8;
            tokoff[tl] = pix;
            const bf16_t* p = qkv + pix * (3L * C) + head * D + lh * 8;
            qf[tl] = *reinterpret_cast<const bf16x8_t*>(p);
            kf[tl] = *reinterpret_cast<const bf16x8_t*>(p + C);
            vf[tl] = *reinterpret_cast<const bf16x8_t*>(p + 2 * C);
            dof[tl] = *reinterpret_cast<const bf16x8_t*>(dout + pix * C + head * D + lh * 8);
        }
        __syncthreads();     // previous window's readers of the LDS tiles are done
#pragma unroll
        for (int tl = 0; tl < 2; ++tl)
#pragma unroll
            for (int e = 0; e < 8; ++e) {          // transposed copies [dim][token]
                const int d = lh * 8 + e, tok = tl * 32 + lr;
                s_kt[d * LP + tok] = (unsigned short)kf[tl][e];
                s_qt[d * LP + tok] = (unsigned short)qf[tl][e];
                s_dot[d * LP + tok] = (unsigned short)dof[tl][e];
            }
        // ---- S^T = K Q^T, dP^T = V dO^T  (one MFMA per 32 x 32 tile: K = 16)
        f32x16_t st[2][2], dp[2][2];
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                f32x16_t z;
#pragma unroll
                for (int r = 0; r < 16; ++r) z[r] = 0.f;
                st[jt][it] = mfma_32x32x16_bf16(kf[jt], qf[it], z);
                dp[jt][it] = mfma_32x32x16_bf16(vf[jt], dof[it], z);
            }
        // ---- softmax over the keys of each query column, dS^T = P^T * (dP^T - rowsum(P * dP))
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            float m = -3.0e38f;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    st[jt][it][r] = st[jt][it][r] * scale + bias[jt][it][r];
                    m = fmaxf(m, st[jt][it][r]);
                }
            m = fmaxf(m, __shfl_xor(m, 32));
            float l = 0.f;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    st[jt][it][r] = __expf(st[jt][it][r] - m);
                    l += st[jt][it][r];
                }
            l += __shfl_xor(l, 32);
            const float inv = 1.f / l;
            float rs = 0.f;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    st[jt][it][r] *= inv;
                    rs = fmaf(st[jt][it][r], dp[jt][it][r], rs);
                }
            rs += __shfl_xor(rs, 32);
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    dp[jt][it][r] = st[jt][it][r] * (dp[jt][it][r] - rs);     // dS^T
                    db[jt][it][r] += dp[jt][it][r];
                }
        }
        // ---- P^T -> LDS [j][i] (bf16), dV^T[d][j] = sum_i dO^T[d][i] P[i][j]
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    s_m[(jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * LP + it * 32 + lr] = f32_to_bf16(st[jt][it][r]);
        __syncthreads();
        f32x16_t dvt[2], dkt[2], dqt[2];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl)
#pragma unroll
            for (int r = 0; r < 16; ++r) dvt[tl][r] = dkt[tl][r] = dqt[tl][r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const bf16x8_t a = lr < D ? *reinterpret_cast<const bf16x8_t*>(&s_dot[lr * LP + kk * 16 + lh * 8]) : zero8;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
                const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(&s_m[(jt * 32 + lr) * LP + kk * 16 + lh * 8]);
                dvt[jt] = mfma_32x32x16_bf16(a, b, dvt[jt]);
            }
        }
        __syncthreads();
        // ---- dS^T -> LDS, dK^T[d][j] = sum_i Q^T[d][i] dS[i][j]
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int it = 0; it < 2; ++it)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    s_m[(jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * LP + it * 32 + lr] = f32_to_bf16(dp[jt][it][r]);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const bf16x8_t a = lr < D ? *reinterpret_cast<const bf16x8_t*>(&s_qt[lr * LP + kk * 16 + lh * 8]) : zero8;
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
                const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(&s_m[(jt * 32 + lr) * LP + kk * 16 + lh * 8]);
                dkt[jt] = mfma_32x32x16_bf16(a, b, dkt[jt]);
            }
        }
        // ---- dQ^T[d][i] = sum_j K^T[d][j] dS^T[j][i]: B straight from the dS^T registers.  k-step (jt, h)
        // covers keys jt*32 + 16h .. +15 in the accumulator's own order: logical k = lh*8 + e <->
        // key jt*32 + 16h + (e&3) + 8*(e>>2) + 4*lh, and the A operand (K^T) is gathered in that order.
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                bf16x8_t a = zero8;
                if (lr < D) {
                    const int j0 = jt * 32 + 16 * h + 4 * lh;
#pragma unroll
                    for (int e = 0; e < 8; ++e) a[e] = (short)s_kt[lr * LP + j0 + (e & 3) + 8 * (e >> 2)];
                }
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    bf16x8_t b;
#pragma unroll
                    for (int e = 0; e < 8; ++e) b[e] = (short)f32_to_bf16(dp[jt][it][8 * h + e]);
                    dqt[it] = mfma_32x32x16_bf16(a, b, dqt[it]);
                }
            }
        // ---- stores: lane (token tl*32 + lr, lh) holds dims 4*lh .. +3 (regs 0-3) and 8 + 4*lh .. +3 (regs 4-7)
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            float* o = dqkv + tokoff[tl] * (3L * C) + head * D + 4 * lh;
            float t4[4];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
#pragma unroll
                for (int e = 0; e < 4; ++e) t4[e] = dqt[tl][4 * g + e] * scale;
                st4(o + 8 * g, t4);
#pragma unroll
                for (int e = 0; e < 4; ++e) t4[e] = dkt[tl][4 * g + e] * scale;
                st4(o + C + 8 * g, t4);
#pragma unroll
                for (int e = 0; e < 4; ++e) t4[e] = dvt[tl][4 * g + e];
                st4(o + 2 * C + 8 * g, t4);
            }
        }
    }
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = jt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, i = it * 32 + lr;
                const long idx = (long)head * T2 * T2 + j * T2 + i;
                if (part) part[(long)blockIdx.x * heads * T2 * T2 + idx] = db[jt][it][r];
                else atomicAdd(dbiasT + idx, db[jt][it][r]);
            }
}

// reflect-padded windows, deterministic mode: dqkv[n, ys, xs, :] += the gradients of the (up to four) padded positions whose
// source pixel is (ys, xs) -- itself, its mirror image in the bottom band, in the right band, in the corner -- in that order
__global__ void __launch_bounds__(256) window_attn_fold_kernel(const float* pad, float* dqkv, int N, int H, int W, int Hp,
                                                               int Wp, int C3) {
    const long total = (long)N * H * W * C3;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C3);
    const long pix = idx / C3;
    const NhwcIdx ix_ = pix_split(pix, W, H);
    const int xs = ix_.x, ys = ix_.y, n = ix_.n;
    const int ym = 2 * H - 2 - ys, xm = 2 * W - 2 - xs;
    const bool my = ym >= H && ym < Hp, mx = xm >= W && xm < Wp;
    const float* base = pad + (long)n * Hp * Wp * C3 + c;
    float t = base[((long)ys * Wp + xs) * C3];
    if (my) t += base[((long)ym * Wp + xs) * C3];
    if (mx) t += base[((long)ys * Wp + xm) * C3];
    if (my && mx) t += base[((long)ym * Wp + xm) * C3];
    dqkv[idx] += t;
}

int window_attn_bwd_impl(const void* qkv, const float* biasT, const void* dout, float* dqkv, float* dbiasT,
                         int N, int H, int W, int C, int heads, int ws, int dtype, hipStream_t s) {
    LEDN_REQUIRE(qkv && biasT && dout && dqkv && dbiasT && N > 0 && H > 0 && W > 0 && C > 0 && heads > 0);
    LEDN_REQUIRE(ws == 8 && C % heads == 0);
    const int D = C / heads;
    const int hh = (H + ws - 1) / ws, ww = (W + ws - 1) / ws;
    LEDN_REQUIRE(hh * ws - H < H && ww * ws - W < W);
    const bool padded = (H % ws) || (W % ws);
    long nb = (long)N * hh * ww;
    if (nb > 256) nb = 256;                                   // wavefronts per head (each walks its windows)
    const long part_floats = nb * heads * 64 * 64;
    const long pad_floats = (padded && det()) ? (long)N * hh * ws * ww * ws * 3 * C : 0;
    float* part = (nb > 8 || det()) ? ws_take(part_floats + pad_floats) : nullptr;
    if (det() && !part) return LEDN_EINVAL;
    float* pad_out = pad_floats ? part + part_floats : nullptr;
    if (!part && nb > 32) nb = 32;                            // atomics fallback: <= 32 per table entry
    const dim3 grid((unsigned)nb, (unsigned)heads);
    if (dtype == LEDN_BF16 && D == 16 && !padded && C % 8 == 0) {   // matrix-core variant
        LEDN_LAUNCH(window_attn_bwd_mfma_kernel, grid, dim3(64), 0, s, (const bf16_t*)qkv, biasT, (const bf16_t*)dout,
                    dqkv, dbiasT, N, H, W, C, heads, hh, ww, part);
        if (part) return finish_partials(part, (int)nb, heads * 64 * 64, 1, dbiasT, nullptr, nullptr, s);
        return check_launch();
    }
    const int rc = with_dtype(dtype, [&](auto t) -> int {
        using T = tag_t<decltype(t)>;
#define LEDN_WB(DD)                                                                                                 \
    do {                                                                                                            \
        if (padded)                                                                                                 \
            LEDN_LAUNCH((window_attn_bwd_kernel<T, DD, true>), grid, dim3(64), 0, s, (const T*)qkv, biasT,          \
                        (const T*)dout, dqkv, dbiasT, N, H, W, C, heads, hh, ww, part, pad_out);                    \
        else                                                                                                        \
            LEDN_LAUNCH((window_attn_bwd_kernel<T, DD, false>), grid, dim3(64), 0, s, (const T*)qkv, biasT,         \
                        (const T*)dout, dqkv, dbiasT, N, H, W, C, heads, hh, ww, part, (float*)nullptr);            \
    } while (0)
        if (D == 16) LEDN_WB(16);
        else if (D == 32) LEDN_WB(32);
        else return LEDN_EINVAL;
#undef LEDN_WB
        return LEDN_OK;
    });
    if (rc != LEDN_OK) return rc;
    if (pad_out) {
        const long total = (long)N * H * W * 3 * C;
        LEDN_LAUNCH(window_attn_fold_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, pad_out, dqkv, N, H, W,
                    hh * ws, ww * ws, 3 * C);
    }
    if (part) return finish_partials(part, (int)nb, heads * 64 * 64, 1, dbiasT, nullptr, nullptr, s);
    return check_launch();
}

// ===========================================================================
// OHEM cross-entropy.
// work layout (floats): prob[P] | loss[P] | u32 hist[3][2048] | u32 state[16]
// state: 0 n_valid, 1 n_correct, 2 rank (remaining), 3 prefix bits, 4 thr bits,
//        5 n_selected, 6 (float) loss_sum
// class_weight (the WT = true instances, cw = [C] floats on the device): loss[p] = cw[y_p] * CE_p in the probability
// pass and the gradient coefficient times cw[y_p] in the backward; prob[], the histograms, the k-th order statistic and
// the masked mean's COUNT never see the weights (ohem_cross_entropy_loss.py:62-90: selection on the probabilities,
// .mean() of the reduction='none' losses).  The WT = false instances are the unweighted code, cw unused.
// ===========================================================================
constexpr int OH_BINS = 2048;
struct OhemWork {
    float* prob;
    float* loss;
    unsigned* hist;
    unsigned* state;
};
__host__ __device__ inline OhemWork ohem_work(float* work, long long P) {
    OhemWork w;
    w.prob = work;
    w.loss = work + P;
    w.hist = reinterpret_cast<unsigned*>(work + 2 * P);
    w.state = w.hist + 3 * OH_BINS;
    return w;
}
long long ohem_work_floats(long long P) { return 2 * P + 3 * OH_BINS + 16; }

__device__ __forceinline__ int oh_bin(unsigned u, int pass) {
    return pass == 0 ? (int)(u >> 21) : (pass == 1 ? (int)((u >> 10) & 2047u) : (int)(u & 1023u));
}

// pass over the pixels: prob of the target class, CE, validity, accuracy, level-0 histogram
template <int CT, bool WT>
__global__ void __launch_bounds__(256) ohem_prob_kernel(const float* logits, const long long* target, long P,
                                                        int C, int ignore_label, float* work, const float* cw) {
    __shared__ unsigned s_hist[OH_BINS];
    __shared__ unsigned s_cnt[2];
    const OhemWork w = ohem_work(work, P);
    for (int i = threadIdx.x; i < OH_BINS; i += blockDim.x) s_hist[i] = 0u;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
        const long long tg = target[p];
        if (tg == ignore_label) {
            w.prob[p] = 2.0f;   // > any probability: never selected
            w.loss[p] = 0.f;
            continue;
        }
        const float* lg = logits + p * C;
        float mx = lg[0];
        int am = 0;
        const int cc = CT > 0 ? CT : C;
#pragma unroll
        for (int c = 1; c < cc; ++c)
            if (lg[c] > mx) { mx = lg[c]; am = c; }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < cc; ++c) se += __expf(lg[c] - mx);
        const float lt = lg[(int)tg] - mx;
        const float pr = __expf(lt) / se;
        w.prob[p] = pr;
        if constexpr (WT) w.loss[p] = cw[(int)tg] * (__logf(se) - lt);
        else w.loss[p] = __logf(se) - lt;
        atomicAdd(&s_hist[oh_bin(__float_as_uint(pr), 0)], 1u);
        atomicAdd(&s_cnt[0], 1u);
        if (am == (int)tg) atomicAdd(&s_cnt[1], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < OH_BINS; i += blockDim.x)
        if (s_hist[i]) atomicAdd(&w.hist[i], s_hist[i]);
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&w.state[threadIdx.x], s_cnt[threadIdx.x]);
}

// single workgroup: locate the bucket holding the wanted rank at this level.  Thread i owns bins
// 8i..8i+7; a block-wide prefix sum of the per-thread counts finds the owner of the rank, which
// then walks its eight bins (the first version walked all 2048 bins with one thread: 75 us).
__global__ void __launch_bounds__(256) ohem_scan_kernel(float* work, long P, int pass, long long min_kept,
                                                        float thres) {
    __shared__ unsigned s_wave[4];
    const OhemWork w = ohem_work(work, P);
    const unsigned nv = w.state[0];
    if (nv == 0u) {   // workgroup-uniform
        if (pass == 0 && threadIdx.x == 0) {
            w.state[4] = __float_as_uint(thres);
            w.state[2] = 0u;
            w.state[3] = 0u;
        }
        return;
    }
    unsigned rank;
    if (pass == 0) {
        const long long k = min_kept < (long long)nv - 1 ? min_kept : (long long)nv - 1;
        rank = (unsigned)k;
    } else {
        rank = w.state[2];
    }
    const unsigned prefix_bits = pass == 0 ? 0u : w.state[3];
    const unsigned* h = w.hist + pass * OH_BINS;
    const int nb = pass == 2 ? 1024 : 2048;
    const int per = nb / 256;
    unsigned hb[8], mine = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        hb[i] = i < per ? h[threadIdx.x * per + i] : 0u;
        mine += hb[i];
    }
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    unsigned incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned nbr = __shfl(incl, lane >= o ? lane - o : lane);
        if (lane >= o) incl += nbr;
    }
    if (lane == 63) s_wave[wid] = incl;
    __syncthreads();          // also orders every thread's reads of state[2..3] before the writes below
    unsigned off = 0u;
    for (int i = 0; i < wid; ++i) off += s_wave[i];
    incl += off;
    const unsigned excl = incl - mine;
    const unsigned total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    int b = -1;
    unsigned r = 0u;
    if (rank >= excl && rank < incl) {          // exactly one thread when rank < total
        r = rank - excl;
        b = threadIdx.x * per;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i >= per || r < hb[i]) break;
            r -= hb[i];
            ++b;
        }
    } else if (rank >= total && threadIdx.x == 255) {   // rank beyond the histogram: last bucket
        r = rank - total;
        b = nb - 1;
    }
    if (b >= 0) {
        const unsigned bits = pass == 0 ? ((unsigned)b << 21) : (pass == 1 ? ((unsigned)b << 10) : (unsigned)b);
        const unsigned full = prefix_bits | bits;
        w.state[3] = full;
        w.state[2] = r;
        if (pass == 2) {
            const float kth = __uint_as_float(full);
            w.state[4] = __float_as_uint(kth > thres ? kth : thres);   // threshold = max(min_value, thresh)
        }
    }
}

__global__ void __launch_bounds__(256) ohem_hist_kernel(float* work, long P, int pass) {
    __shared__ unsigned s_hist[OH_BINS];
    const OhemWork w = ohem_work(work, P);
    for (int i = threadIdx.x; i < OH_BINS; i += blockDim.x) s_hist[i] = 0u;
    __syncthreads();
    const unsigned prefix = w.state[3];
    const unsigned mask = pass == 1 ? 0xffe00000u : 0xfffffc00u;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
        const unsigned u = __float_as_uint(w.prob[p]);
        if ((u & mask) == prefix) atomicAdd(&s_hist[oh_bin(u, pass)], 1u);
    }
    __syncthreads();
    unsigned* h = w.hist + pass * OH_BINS;
    for (int i = threadIdx.x; i < OH_BINS; i += blockDim.x)
        if (s_hist[i]) atomicAdd(&h[i], s_hist[i]);
}

// part (deterministic mode): one (sum, count) row per workgroup instead of the two atomics; ohem_final_kernel adds the rows
// in row order
__global__ void __launch_bounds__(256) ohem_reduce_kernel(float* work, long P, float* part) {
    __shared__ float s_sum[4];
    __shared__ unsigned s_cnt[4];
    const OhemWork w = ohem_work(work, P);
    const float thr = __uint_as_float(w.state[4]);
    float sum = 0.f;
    unsigned cnt = 0u;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
        if (w.prob[p] < thr) {
            sum += w.loss[p];
            ++cnt;
        }
    }
    sum = wave_sum(sum);
    float cf = wave_sum((float)cnt);   // exact below 2^24 per wave
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_cnt[threadIdx.x >> 6] = (unsigned)cf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float bs = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        const unsigned bc = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (part) {
            part[2 * blockIdx.x] = bs;
            part[2 * blockIdx.x + 1] = __uint_as_float(bc);
        } else {
            atomicAdd(reinterpret_cast<float*>(&w.state[6]), bs);
            atomicAdd(&w.state[5], bc);
        }
    }
}

__global__ void ohem_final_kernel(float* work, long P, float loss_weight, float* out, const float* part, int nparts) {
    const OhemWork w = ohem_work(work, P);
    const unsigned nv = w.state[0];
    unsigned nsel = w.state[5];
    float sum = __uint_as_float(w.state[6]);
    if (part) {
        sum = 0.f;
        nsel = 0u;
        for (int b = 0; b < nparts; ++b) {
            sum += part[2 * b];
            nsel += __float_as_uint(part[2 * b + 1]);
        }
    }
    out[0] = nv == 0u ? 0.f : loss_weight * (sum / (float)nsel);   // 0/0 -> NaN like the reference
    const float eps = 1.1920929e-07f;
    out[1] = ((float)w.state[1] + eps) * (100.0f / ((float)nv + eps));
    out[2] = __uint_as_float(w.state[4]);
    out[3] = (float)nsel;
}

int ohem_ce_fwd_impl(const float* logits, const long long* target, long long P, int C, float thres,
                     long long min_kept, float loss_weight, int ignore_label, const float* cw, float* work,
                     float* out, hipStream_t s) {
    LEDN_REQUIRE(logits && target && work && out && P > 0 && C > 1 && min_kept >= 1);
    LEDN_REQUIRE(P < (1LL << 31));
    const OhemWork w = ohem_work(work, P);
    if (hipMemsetAsync(w.hist, 0, sizeof(unsigned) * (3 * OH_BINS + 16), s) != hipSuccess) return LEDN_ELAUNCH;
    const dim3 grid((unsigned)(cdiv(P, 256) < 2048 ? cdiv(P, 256) : 2048));
    if (cw) {
        if (C == 2) LEDN_LAUNCH((ohem_prob_kernel<2, true>), grid, dim3(256), 0, s, logits, target, (long)P, C, ignore_label, work, cw);
        else LEDN_LAUNCH((ohem_prob_kernel<0, true>), grid, dim3(256), 0, s, logits, target, (long)P, C, ignore_label, work, cw);
    } else {
        if (C == 2) LEDN_LAUNCH((ohem_prob_kernel<2, false>), grid, dim3(256), 0, s, logits, target, (long)P, C, ignore_label, work, cw);
        else LEDN_LAUNCH((ohem_prob_kernel<0, false>), grid, dim3(256), 0, s, logits, target, (long)P, C, ignore_label, work, cw);
    }
    LEDN_LAUNCH(ohem_scan_kernel, dim3(1), dim3(256), 0, s, work, (long)P, 0, min_kept, thres);
    LEDN_LAUNCH(ohem_hist_kernel, grid, dim3(256), 0, s, work, (long)P, 1);
    LEDN_LAUNCH(ohem_scan_kernel, dim3(1), dim3(256), 0, s, work, (long)P, 1, min_kept, thres);
    LEDN_LAUNCH(ohem_hist_kernel, grid, dim3(256), 0, s, work, (long)P, 2);
    LEDN_LAUNCH(ohem_scan_kernel, dim3(1), dim3(256), 0, s, work, (long)P, 2, min_kept, thres);
    // deterministic mode: no float atomics.  The rows overlay the workspace base like every two-stage reduction: nothing is
    // pending there -- deferred BatchNorm rows live only between a producer and the bn_finalize that follows it at once
    // (include/ledn.h, ledn_conv2d_deferred_stats), and no loss sits between such a pair
    float* part = det() ? ws_take(2L * grid.x) : nullptr;
    if (det() && !part) return LEDN_EINVAL;
    LEDN_LAUNCH(ohem_reduce_kernel, grid, dim3(256), 0, s, work, (long)P, part);
    LEDN_LAUNCH(ohem_final_kernel, dim3(1), dim3(1), 0, s, work, (long)P, loss_weight, out, (const float*)part, (int)grid.x);
    return check_launch();
}

template <int CT, bool WT>
__global__ void __launch_bounds__(256) ohem_bwd_kernel(const float* logits, const long long* target, long P,
                                                       int C, int ignore_label, const float* work,
                                                       const float* out, const float* dloss,
                                                       float loss_weight, float* dlogits, const float* cw) {
    const float* prob = work;
    const float thr = out[2];
    const float coef = dloss[0] * loss_weight / out[3];
    const long stride = (long)gridDim.x * blockDim.x;
    const int cc = CT > 0 ? CT : C;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
        const long long tg = target[p];
        float* dl = dlogits + p * C;
        if (tg == ignore_label || !(prob[p] < thr)) {
#pragma unroll
            for (int c = 0; c < cc; ++c) dl[c] = 0.f;
            continue;
        }
        const float* lg = logits + p * C;
        float mx = lg[0];
#pragma unroll
        for (int c = 1; c < cc; ++c) mx = fmaxf(mx, lg[c]);
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < cc; ++c) se += __expf(lg[c] - mx);
        const float inv = 1.f / se;
        const float cf = WT ? coef * cw[(int)tg] : coef;
#pragma unroll
        for (int c = 0; c < cc; ++c)
            dl[c] = cf * (__expf(lg[c] - mx) * inv - (c == (int)tg ? 1.f : 0.f));
    }
}

int ohem_ce_bwd_impl(const float* logits, const long long* target, long long P, int C, int ignore_label,
                     const float* work, const float* out, const float* dloss, float loss_weight,
                     const float* cw, float* dlogits, hipStream_t s) {
    LEDN_REQUIRE(logits && target && work && out && dloss && dlogits && P > 0 && C > 1);
    const dim3 grid((unsigned)(cdiv(P, 256) < 4096 ? cdiv(P, 256) : 4096));
    if (cw) {
        if (C == 2)
            LEDN_LAUNCH((ohem_bwd_kernel<2, true>), grid, dim3(256), 0, s, logits, target, (long)P, C, ignore_label, work,
                        out, dloss, loss_weight, dlogits, cw);
        else
            LEDN_LAUNCH((ohem_bwd_kernel<0, true>), grid, dim3(256), 0, s, logits, target, (long)P, C, ignore_label, work,
                        out, dloss, loss_weight, dlogits, cw);
    } else if (C == 2)
        LEDN_LAUNCH((ohem_bwd_kernel<2, false>), grid, dim3(256), 0, s, logits, target, (long)P, C, ignore_label, work,
                    out, dloss, loss_weight, dlogits, cw);
    else
        LEDN_LAUNCH((ohem_bwd_kernel<0, false>), grid, dim3(256), 0, s, logits, target, (long)P, C, ignore_label, work,
                    out, dloss, loss_weight, dlogits, cw);
    return check_launch();
}

// ---------------------------------------------------------------------------
// OHEM-CE on logits that are the bilinear (align_corners=False) upsampling of src [N,Hs,Ws,2] to H x W, without
// materialising them: LEDHead.loss_by_feat resizes each fused output to the label size right in front of the loss
// (led_head.py:132-138); at 16 x 1024^2 that tensor and its gradient are 134 MB each, written once and read twice.
// Forward: ohem_prob with the four-tap interpolation in front (any ratio).  Backward (exact 2x): a workgroup owns a
// 16 x 16 tile of src; the softmax gradients of its 34 x 34 children are formed once in LDS, then every src pixel
// gathers its 4 x 4 children with the interpolation weights (the adjoint of the resize), so neither dlogits nor a
// scatter with atomics exists.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void up_logits2(const float* src, int Ws, const Lerp& ly, const Lerp& lx, float& l0, float& l1) {
    const float2 v00 = *reinterpret_cast<const float2*>(src + ((long)ly.i0 * Ws + lx.i0) * 2);
    const float2 v01 = *reinterpret_cast<const float2*>(src + ((long)ly.i0 * Ws + lx.i1) * 2);
    const float2 v10 = *reinterpret_cast<const float2*>(src + ((long)ly.i1 * Ws + lx.i0) * 2);
    const float2 v11 = *reinterpret_cast<const float2*>(src + ((long)ly.i1 * Ws + lx.i1) * 2);
    l0 = ly.w0 * (lx.w0 * v00.x + lx.w1 * v01.x) + ly.w1 * (lx.w0 * v10.x + lx.w1 * v11.x);
    l1 = ly.w0 * (lx.w0 * v00.y + lx.w1 * v01.y) + ly.w1 * (lx.w0 * v10.y + lx.w1 * v11.y);
}

template <bool WT>
__global__ void __launch_bounds__(256) ohem_prob_up_kernel(const float* src, int N, int Hs, int Ws, int H, int W,
                                                           const long long* target, int ignore_label, float* work,
                                                           const float* cw) {
    __shared__ unsigned s_hist[OH_BINS];
    __shared__ unsigned s_cnt[2];
    const long P = (long)N * H * W;
    const OhemWork w = ohem_work(work, P);
    for (int i = threadIdx.x; i < OH_BINS; i += blockDim.x) s_hist[i] = 0u;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
        const long long tg = target[p];
        if (tg == ignore_label) {
            w.prob[p] = 2.0f;
            w.loss[p] = 0.f;
            continue;
        }
        const int x = (int)(p % W), y = (int)((p / W) % H), n = (int)(p / ((long)W * H));
        float lg[2];
        up_logits2(src + (long)n * Hs * Ws * 2, Ws, lerp_coord(y, Hs, H), lerp_coord(x, Ws, W), lg[0], lg[1]);
        const int am = lg[1] > lg[0] ? 1 : 0;
        const float mx = lg[am];
        const float se = __expf(lg[0] - mx) + __expf(lg[1] - mx);
        const float lt = lg[(int)tg] - mx;
        const float pr = __expf(lt) / se;
        w.prob[p] = pr;
        if constexpr (WT) w.loss[p] = cw[(int)tg] * (__logf(se) - lt);
        else w.loss[p] = __logf(se) - lt;
        atomicAdd(&s_hist[oh_bin(__float_as_uint(pr), 0)], 1u);
        atomicAdd(&s_cnt[0], 1u);
        if (am == (int)tg) atomicAdd(&s_cnt[1], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < OH_BINS; i += blockDim.x)
        if (s_hist[i]) atomicAdd(&w.hist[i], s_hist[i]);
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&w.state[threadIdx.x], s_cnt[threadIdx.x]);
}

int ohem_ce_up_fwd_impl(const float* src, int N, int Hs, int Ws, int H, int W, const long long* target, float thres,
                        long long min_kept, float loss_weight, int ignore_label, const float* cw, float* work,
                        float* out, hipStream_t s) {
    LEDN_REQUIRE(src && target && work && out && N > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0);
    const long long P = (long long)N * H * W;
    LEDN_REQUIRE(P < (1LL << 31) && min_kept >= 1);
    const OhemWork w = ohem_work(work, P);
    if (hipMemsetAsync(w.hist, 0, sizeof(unsigned) * (3 * OH_BINS + 16), s) != hipSuccess) return LEDN_ELAUNCH;
    const dim3 grid((unsigned)(cdiv(P, 256) < 2048 ? cdiv(P, 256) : 2048));
    if (cw) LEDN_LAUNCH(ohem_prob_up_kernel<true>, grid, dim3(256), 0, s, src, N, Hs, Ws, H, W, target, ignore_label, work, cw);
    else LEDN_LAUNCH(ohem_prob_up_kernel<false>, grid, dim3(256), 0, s, src, N, Hs, Ws, H, W, target, ignore_label, work, cw);
    LEDN_LAUNCH(ohem_scan_kernel, dim3(1), dim3(256), 0, s, work, (long)P, 0, min_kept, thres);
    LEDN_LAUNCH(ohem_hist_kernel, grid, dim3(256), 0, s, work, (long)P, 1);
    LEDN_LAUNCH(ohem_scan_kernel, dim3(1), dim3(256), 0, s, work, (long)P, 1, min_kept, thres);
    LEDN_LAUNCH(ohem_hist_kernel, grid, dim3(256), 0, s, work, (long)P, 2);
    LEDN_LAUNCH(ohem_scan_kernel, dim3(1), dim3(256), 0, s, work, (long)P, 2, min_kept, thres);
    // deterministic mode: no float atomics.  The rows overlay the workspace base like every two-stage reduction: nothing is
    // pending there -- deferred BatchNorm rows live only between a producer and the bn_finalize that follows it at once
    // (include/ledn.h, ledn_conv2d_deferred_stats), and no loss sits between such a pair
    float* part = det() ? ws_take(2L * grid.x) : nullptr;
    if (det() && !part) return LEDN_EINVAL;
    LEDN_LAUNCH(ohem_reduce_kernel, grid, dim3(256), 0, s, work, (long)P, part);
    LEDN_LAUNCH(ohem_final_kernel, dim3(1), dim3(1), 0, s, work, (long)P, loss_weight, out, (const float*)part, (int)grid.x);
    return check_launch();
}

template <bool WT>
__global__ void __launch_bounds__(256) ohem_bwd_up2_kernel(const float* src, int N, int Hs, int Ws,
                                                           const long long* target, int ignore_label,
                                                           const float* work, const float* out, const float* dloss,
                                                           float loss_weight, float* dsrc, const float* cw) {
    constexpr int T = 16, CH = 2 * T + 2;                   // src tile, children per side
    __shared__ float2 s_g[CH * CH];
    const int H = 2 * Hs, W = 2 * Ws;
    const int tw = (Ws + T - 1) / T, th = (Hs + T - 1) / T;
    const int bj = blockIdx.x % tw, bi = (blockIdx.x / tw) % th, n = blockIdx.x / (tw * th);
    const int i0 = bi * T, j0 = bj * T;
    const float* prob = work;
    const float thr = out[2];
    const float coef = dloss[0] * loss_weight / out[3];
    const float* sn = src + (long)n * Hs * Ws * 2;
    for (int k = threadIdx.x; k < CH * CH; k += 256) {
        const int y = 2 * i0 - 1 + k / CH, x = 2 * j0 - 1 + k % CH;
        float2 g = make_float2(0.f, 0.f);
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const long p = ((long)n * H + y) * W + x;
            const long long tg = target[p];
            if (tg != ignore_label && prob[p] < thr) {
                float l0, l1;
                up_logits2(sn, Ws, lerp_coord(y, Hs, H), lerp_coord(x, Ws, W), l0, l1);
                const float mx = fmaxf(l0, l1);
                const float e0 = __expf(l0 - mx), e1 = __expf(l1 - mx), inv = 1.f / (e0 + e1);
                const float cf = WT ? coef * cw[(int)tg] : coef;
                g.x = cf * (e0 * inv - (tg == 0 ? 1.f : 0.f));
                g.y = cf * (e1 * inv - (tg == 1 ? 1.f : 0.f));
            }
        }
        s_g[k] = g;
    }
    __syncthreads();
    const int a = threadIdx.x / T, b = threadIdx.x % T, i = i0 + a, j = j0 + b;
    if (i >= Hs || j >= Ws) return;
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
        const int y = 2 * i - 1 + dy;
        if (y < 0 || y >= H) continue;
        const Lerp ly = lerp_coord(y, Hs, H);
        const float wy = (ly.i0 == i ? ly.w0 : 0.f) + (ly.i1 == i ? ly.w1 : 0.f);
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) {
            const int x = 2 * j - 1 + dx;
            if (x < 0 || x >= W) continue;
            const Lerp lx = lerp_coord(x, Ws, W);
            const float wgt = wy * ((lx.i0 == j ? lx.w0 : 0.f) + (lx.i1 == j ? lx.w1 : 0.f));
            const float2 g = s_g[(2 * a + dy) * CH + 2 * b + dx];
            acc.x += wgt * g.x;
            acc.y += wgt * g.y;
        }
    }
    *reinterpret_cast<float2*>(dsrc + (((long)n * Hs + i) * Ws + j) * 2) = acc;
}

int ohem_ce_up_bwd_impl(const float* src, int N, int Hs, int Ws, int H, int W, const long long* target,
                        int ignore_label, const float* work, const float* out, const float* dloss, float loss_weight,
                        const float* cw, float* dsrc, hipStream_t s) {
    LEDN_REQUIRE(src && target && work && out && dloss && dsrc && N > 0 && Hs > 0 && Ws > 0);
    LEDN_REQUIRE(H == 2 * Hs && W == 2 * Ws);               // the fused adjoint is written for the exact 2x resize
    const long nb = (long)N * cdiv(Hs, 16) * cdiv(Ws, 16);
    LEDN_REQUIRE(nb < (1L << 31));
    if (cw)
        LEDN_LAUNCH(ohem_bwd_up2_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, src, N, Hs, Ws, target, ignore_label, work,
                    out, dloss, loss_weight, dsrc, cw);
    else
        LEDN_LAUNCH(ohem_bwd_up2_kernel<false>, dim3((unsigned)nb), dim3(256), 0, s, src, N, Hs, Ws, target, ignore_label, work,
                    out, dloss, loss_weight, dsrc, cw);
    return check_launch();
}

// ===========================================================================
// multi-tensor SGD: grid = (chunks, tensors)
// ===========================================================================
__global__ void __launch_bounds__(256) sgd_kernel(const ledn_sgd_entry* table, float lr_arg, const float* lr_dev,
                                                  float momentum, float wd, float gscale) {
    const float lr = lr_dev ? *lr_dev : lr_arg;   // device-resident lr: a captured graph replays with a new value
    const ledn_sgd_entry e = table[blockIdx.y];
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < e.n; i += stride) {
        const float p = e.p[i];
        const float g = e.g[i] * gscale + wd * p;
        const float m = momentum * e.m[i] + g;
        e.m[i] = m;
        e.p[i] = p - lr * m;
        e.g[i] = 0.f;
    }
}

int sgd_step_impl(const ledn_sgd_entry* table_dev, int n_tensors, long long max_n, float lr,
                  const float* lr_dev, float momentum, float weight_decay, float grad_scale, hipStream_t s) {
    LEDN_REQUIRE(table_dev && n_tensors > 0 && max_n > 0);
    long chunks = cdiv(max_n, 256 * 8);
    if (chunks > 64) chunks = 64;
    LEDN_LAUNCH(sgd_kernel, dim3((unsigned)chunks, (unsigned)n_tensors), dim3(256), 0, s, table_dev, lr,
                lr_dev, momentum, weight_decay, grad_scale);
    return check_launch();
}

// ===========================================================================
// gradient clipping (mmengine OptimWrapper clip_grad = torch.nn.utils.clip_grad_norm_ / clip_grad_value_), folded into the
// SGD launch.  Pass 1 (grad_norm_partials_kernel): one float per workgroup over the flat gradient buffer -- the sum of
// squares (L2) or the largest magnitude (inf).  Pass 2 (sgd_clip_kernel): every workgroup sums the <= 256 partials itself
// in its prologue (the launch boundary is the grid-wide barrier; no finish launch, no ticket), forms the coefficient and
// runs the SGD update with grad_scale * coef.  No atomics anywhere and one fixed combining order: the norm is the same
// bits from run to run and in every workgroup, with or without deterministic mode.
// ===========================================================================
// torch.max semantics: a NaN on either side wins (fmaxf would drop it)
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

template <bool INF> __device__ __forceinline__ float norm_acc(float acc, float v) {
    if constexpr (INF) return nan_max(acc, fabsf(v));
    else return acc + v * v;
}
template <bool INF> __device__ __forceinline__ float norm_acc4(float acc, const float4& v) {
    return norm_acc<INF>(norm_acc<INF>(norm_acc<INF>(norm_acc<INF>(acc, v.x), v.y), v.z), v.w);
}
// combines one value per thread of a 256-thread workgroup: xor butterfly inside each wave, then the four wave results in
// wave order through LDS.  Every thread returns the same bits.  (Both operations are commutative, so the butterfly leaves
// one value in all 64 lanes.)
template <bool INF> __device__ __forceinline__ float block256_combine(float v, float* s_w) {
    if constexpr (INF) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v = nan_max(v, __shfl_xor(v, m));
    } else {
        v = wave_sum(v);
    }
    if (lane_id() == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = s_w[0];
    if constexpr (INF) r = nan_max(nan_max(nan_max(r, s_w[1]), s_w[2]), s_w[3]);
    else r = ((r + s_w[1]) + s_w[2]) + s_w[3];
    return r;
}

// grid-stride over the 16-byte vectors of g[head .. head + 4 nvec) (head = the 0-3 floats in front of the first aligned
// address); the head and the 0-3 tail floats go to the first threads of workgroup 0.  The loop body takes four vectors per
// trip so that four loads are in flight, and accumulates them in index order: the same sum as one vector per trip.
template <bool INF>
__global__ void __launch_bounds__(256) grad_norm_partials_kernel(const float* g, long n, int head, float* partials) {
    __shared__ float s_w[4];
    const int t = threadIdx.x;
    const long nvec = (n - head) >> 2;
    const int tail = (int)(n - head - (nvec << 2));
    const float4* gv = reinterpret_cast<const float4*>(g + head);
    const long stride = (long)gridDim.x * 256;
    float acc = 0.f;
    long v = (long)blockIdx.x * 256 + t;
    for (; v + 3 * stride < nvec; v += 4 * stride) {
        const float4 a = gv[v], b = gv[v + stride], c = gv[v + 2 * stride], d = gv[v + 3 * stride];
        acc = norm_acc4<INF>(norm_acc4<INF>(norm_acc4<INF>(norm_acc4<INF>(acc, a), b), c), d);
    }
    for (; v < nvec; v += stride) acc = norm_acc4<INF>(acc, gv[v]);
    if (blockIdx.x == 0) {
        if (t < head) acc = norm_acc<INF>(acc, g[t]);
        if (t < tail) acc = norm_acc<INF>(acc, g[head + (nvec << 2) + t]);
    }
    acc = block256_combine<INF>(acc, s_w);
    if (t == 0) partials[blockIdx.x] = acc;
}

int grad_norm_partials_impl(const float* g, long long n, int norm_type, float* partials, int n_partials, hipStream_t s) {
    LEDN_REQUIRE(g && partials && n > 0 && ((uintptr_t)g & 3u) == 0);
    LEDN_REQUIRE(n_partials >= 1 && n_partials <= LEDN_CLIP_MAX_PARTIALS);
    LEDN_REQUIRE(norm_type == LEDN_NORM_L2 || norm_type == LEDN_NORM_INF);
    long head = (long)((16u - ((uintptr_t)g & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    if (norm_type == LEDN_NORM_INF)
        LEDN_LAUNCH(grad_norm_partials_kernel<true>, dim3((unsigned)n_partials), dim3(256), 0, s, g, (long)n, (int)head, partials);
    else
        LEDN_LAUNCH(grad_norm_partials_kernel<false>, dim3((unsigned)n_partials), dim3(256), 0, s, g, (long)n, (int)head, partials);
    return check_launch();
}

// MODE: LEDN_NORM_L2 / LEDN_NORM_INF = clip by the total norm behind `partials`, LEDN_NORM_NONE = clip by value.
// (sgd_kernel above stays the unclipped instance, untouched.)
template <int MODE>
__global__ void __launch_bounds__(256) sgd_clip_kernel(const ledn_sgd_entry* table, float lr_arg, const float* lr_dev,
                                                       float momentum, float wd, float gscale, const float* partials,
                                                       int n_partials, float max_norm, float clip_value, float* norm_out) {
    const ledn_sgd_entry e = table[blockIdx.y];
    if ((long)blockIdx.x * blockDim.x >= e.n) return;      // (whole workgroup: nothing of this tensor is its to update)
    const float lr = lr_dev ? *lr_dev : lr_arg;
    float gs = gscale;
    if constexpr (MODE != LEDN_NORM_NONE) {
        __shared__ float s_w[4];
        const int t = threadIdx.x;
        float tot = block256_combine<MODE == LEDN_NORM_INF>(t < n_partials ? partials[t] : 0.f, s_w);
        if constexpr (MODE == LEDN_NORM_L2) tot = sqrtf(tot);
        tot *= gscale;                                     // the norm of the gradient the update uses (DDP's mean)
        const float c = max_norm / (tot + 1e-6f);
        const float coef = c > 1.f ? 1.f : c;              // torch.clamp(max=1): a NaN coefficient stays NaN
        if (norm_out && blockIdx.x == 0 && blockIdx.y == 0 && t == 0) {
            norm_out[0] = tot;
            norm_out[1] = coef;
        }
        gs = gscale * coef;
    }
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < e.n; i += stride) {
        const float p = e.p[i];
        float g;
        if constexpr (MODE == LEDN_NORM_NONE) {
            const float sg = e.g[i] * gs;
            g = (sg < -clip_value ? -clip_value : (sg > clip_value ? clip_value : sg)) + wd * p;   // torch.clamp: NaN passes
        } else {
            g = e.g[i] * gs + wd * p;
        }
        const float m = momentum * e.m[i] + g;
        e.m[i] = m;
        e.p[i] = p - lr * m;
        e.g[i] = 0.f;
    }
}

int sgd_step_clip_impl(const ledn_sgd_entry* table_dev, int n_tensors, long long max_n, float lr, const float* lr_dev,
                       float momentum, float weight_decay, float grad_scale, const float* partials, int n_partials,
                       int norm_type, float max_norm, float clip_value, float* norm_out, hipStream_t s) {
    LEDN_REQUIRE(table_dev && n_tensors > 0 && max_n > 0);
    LEDN_REQUIRE(norm_type == LEDN_NORM_L2 || norm_type == LEDN_NORM_INF || norm_type == LEDN_NORM_NONE);
    if (norm_type == LEDN_NORM_NONE) {
        LEDN_REQUIRE(clip_value > 0.f);
    } else {
        LEDN_REQUIRE(partials && n_partials >= 1 && n_partials <= LEDN_CLIP_MAX_PARTIALS && max_norm > 0.f);
    }
    long chunks = cdiv(max_n, 256 * 8);
    if (chunks > 64) chunks = 64;
    const dim3 grid((unsigned)chunks, (unsigned)n_tensors);
#define LEDN_SGD_CLIP(MODE)                                                                                          \
    LEDN_LAUNCH(sgd_clip_kernel<MODE>, grid, dim3(256), 0, s, table_dev, lr, lr_dev, momentum, weight_decay, grad_scale, \
                partials, n_partials, max_norm, clip_value, norm_out)
    if (norm_type == LEDN_NORM_L2) LEDN_SGD_CLIP(LEDN_NORM_L2);
    else if (norm_type == LEDN_NORM_INF) LEDN_SGD_CLIP(LEDN_NORM_INF);
    else LEDN_SGD_CLIP(LEDN_NORM_NONE);
#undef LEDN_SGD_CLIP
    return check_launch();
}

// ===========================================================================
// generalised multi-tensor optimizer step (ledn_optim_step): SGD or AdamW, a learning-rate and a weight-decay multiplier
// per tensor (mmengine paramwise_cfg), the rate as lr_mult * A + B (A, B: the two scalars every supported schedule
// collapses to), clipping folded in as in sgd_clip_kernel.  grid = (chunks, tensors) as sgd_kernel.  A tensor whose
// p / g / m / v pointers are all 16-byte aligned moves as float4 (the 0-3 tail floats go to the first threads of chunk 0);
// any other tensor takes the scalar loop.  Both paths run the same per-element expressions, so the path taken never
// changes a bit.  No atomics, no cross-workgroup reduction: the same bits on every run in both determinism modes.
// (sgd_kernel / sgd_clip_kernel above stay what a plain SGD configuration launches, untouched.)
// ===========================================================================
enum { OPT_CLIP_OFF = 0, OPT_CLIP_L2 = 1, OPT_CLIP_INF = 2, OPT_CLIP_VALUE = 3 };

struct OptimArgs {
    const ledn_optim_entry* table;
    const float* sched_dev;            // NULL or {A, B, bc1, sqrt(bc2)} on the device (a captured graph replays the schedule)
    float A, B, bc1, sbc2;
    float momentum, b1, omb1, b2, omb2, eps;
    float weight_decay, gscale;
    const float* partials;
    int n_partials;
    float max_norm, clip_value;
    float* norm_out;
};

struct OptimConsts {                   // per tensor, per thread: formed once in front of the loop
    float gs, cv, lr, wd, mom, decay, b1, omb1, b2, omb2, step, sbc2, eps;
};

// The roundings are written out, not left to -ffp-contract: which product the compiler fuses into which sum depends on the
// loop around the expression (sgd_kernel's a * b + c * d + e * f comes out as rn(mom * m) + fma(gs, g, rn(wd * p)), the same
// text inside another loop does not), and the SGD form has to give the bits of sgd_kernel / sgd_clip_kernel from the float4
// loop and the scalar loop alike.  The emulator's host compiler fuses nothing, there and here.
#ifdef LEDN_CPU_EMU
__device__ __forceinline__ float opt_fma(float a, float b, float c) { return a * b + c; }
#else
__device__ __forceinline__ float opt_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
#endif
__device__ __forceinline__ float opt_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float opt_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

template <int KIND, int CLIP>
__device__ __forceinline__ void optim_update(const OptimConsts& c, float& p, float g, float& m, float& v) {
    if constexpr (KIND == LEDN_OPTIM_SGD) {
        const float wp = opt_mul(c.wd, p);
        float gg;
        if constexpr (CLIP == OPT_CLIP_VALUE) {
            const float sg = opt_mul(g, c.gs);
            gg = opt_add(wp, sg < -c.cv ? -c.cv : (sg > c.cv ? c.cv : sg));       // torch.clamp: NaN passes
        } else {
            gg = opt_fma(g, c.gs, wp);
        }
        m = opt_add(opt_mul(c.mom, m), gg);
        p = opt_fma(-c.lr, m, p);
    } else {
        float sg = opt_mul(g, c.gs);
        if constexpr (CLIP == OPT_CLIP_VALUE) sg = sg < -c.cv ? -c.cv : (sg > c.cv ? c.cv : sg);
        p = opt_mul(p, c.decay);
        m = opt_fma(c.b1, m, opt_mul(c.omb1, sg));
        v = opt_fma(c.b2, v, opt_mul(c.omb2, opt_mul(sg, sg)));
        p = opt_add(p, -(opt_mul(c.step, m) / opt_add(sqrtf(v) / c.sbc2, c.eps)));
    }
}

template <int KIND, int CLIP>
__global__ void __launch_bounds__(256) optim_kernel(const OptimArgs a) {
    const ledn_optim_entry e = a.table[blockIdx.y];
    const bool vec = ((((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v) & 15u) == 0) && e.n >= 4;
    // (whole workgroup: nothing of this tensor is its to update; chunk 0 always stays, it owns the tail)
    if ((long)blockIdx.x * blockDim.x * (vec ? 4 : 1) >= e.n) return;
    const int t = threadIdx.x;
    float A = a.A, B = a.B, bc1 = a.bc1, sbc2 = a.sbc2;
    if (a.sched_dev) {
        A = a.sched_dev[0];
        B = a.sched_dev[1];
        if constexpr (KIND == LEDN_OPTIM_ADAMW) {
            bc1 = a.sched_dev[2];
            sbc2 = a.sched_dev[3];
        }
    }
    OptimConsts c;
    c.gs = a.gscale;
    if constexpr (CLIP == OPT_CLIP_L2 || CLIP == OPT_CLIP_INF) {
        __shared__ float s_w[4];
        float tot = block256_combine<CLIP == OPT_CLIP_INF>(t < a.n_partials ? a.partials[t] : 0.f, s_w);
        if constexpr (CLIP == OPT_CLIP_L2) tot = sqrtf(tot);
        tot *= a.gscale;                                   // the norm of the gradient the update uses (DDP's mean)
        const float q = a.max_norm / (tot + 1e-6f);
        const float coef = q > 1.f ? 1.f : q;              // torch.clamp(max=1): a NaN coefficient stays NaN
        if (a.norm_out && blockIdx.x == 0 && blockIdx.y == 0 && t == 0) {
            a.norm_out[0] = tot;
            a.norm_out[1] = coef;
        }
        c.gs = a.gscale * coef;
    }
    c.cv = a.clip_value;
    c.lr = e.lr_mult * A + B;
    c.wd = e.wd_mult * a.weight_decay;
    c.mom = a.momentum;
    c.decay = 1.f - c.lr * c.wd;
    c.b1 = a.b1, c.omb1 = a.omb1, c.b2 = a.b2, c.omb2 = a.omb2;
    c.step = c.lr / bc1;
    c.sbc2 = sbc2;
    c.eps = a.eps;
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + t;
    if (vec) {
        const long nvec = e.n >> 2;
        float4* pv = reinterpret_cast<float4*>(e.p);
        float4* gv = reinterpret_cast<float4*>(e.g);
        float4* mv = reinterpret_cast<float4*>(e.m);
        float4* vv = reinterpret_cast<float4*>(e.v);
        for (long i = i0; i < nvec; i += stride) {
            float4 p = pv[i], m = mv[i], v = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 g = gv[i];
            if constexpr (KIND == LEDN_OPTIM_ADAMW) v = vv[i];
            optim_update<KIND, CLIP>(c, p.x, g.x, m.x, v.x);
            optim_update<KIND, CLIP>(c, p.y, g.y, m.y, v.y);
            optim_update<KIND, CLIP>(c, p.z, g.z, m.z, v.z);
            optim_update<KIND, CLIP>(c, p.w, g.w, m.w, v.w);
            mv[i] = m;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) vv[i] = v;
            pv[i] = p;
            gv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const long done = nvec << 2;
        if (blockIdx.x == 0 && done + t < e.n) {
            const long i = done + t;
            float p = e.p[i], m = e.m[i], v = 0.f;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) v = e.v[i];
            optim_update<KIND, CLIP>(c, p, e.g[i], m, v);
            e.m[i] = m;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) e.v[i] = v;
            e.p[i] = p;
            e.g[i] = 0.f;
        }
    } else {
        for (long i = i0; i < e.n; i += stride) {
            float p = e.p[i], m = e.m[i], v = 0.f;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) v = e.v[i];
            optim_update<KIND, CLIP>(c, p, e.g[i], m, v);
            e.m[i] = m;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) e.v[i] = v;
            e.p[i] = p;
            e.g[i] = 0.f;
        }
    }
}

// weight averaging folded into the launch (ledn_optim_step_ema): avg <- avg + w * (p_new - avg) by the thread that formed
// p_new.  w >= 1 (the hook's first step, or an iteration before begin_iter) is a copy: p_new itself is stored and avg is
// not read -- avg + 1 * (p - avg) is not p in f32, and an uninitialised or non-finite avg would come out NaN.
__device__ __forceinline__ float ema_lerp(float w, float avg, float p) { return opt_fma(w, opt_add(p, -avg), avg); }

// optim_kernel with the averaged column.  A kernel of its own and not a template switch on optim_kernel: routing the
// shared body through a helper changed the code of the existing launch (flat instead of global accesses, other fused
// products), and ledn_optim_step has to stay what it was.  Everything up to the store of p is optim_kernel's text.
template <int KIND, int CLIP>
__global__ void __launch_bounds__(256) optim_ema_kernel(const OptimArgs a, float* const* avgs, float w_arg, const float* w_dev) {
    const ledn_optim_entry e = a.table[blockIdx.y];
    float* const avg = avgs[blockIdx.y];
    const bool vec = ((((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v | (uintptr_t)avg) & 15u) == 0) && e.n >= 4;
    const float ema_w = w_dev ? *w_dev : w_arg;            // device-resident w: a captured graph replays with a new value
    const bool ema_copy = ema_w >= 1.f;                    // (the same in every thread of the grid)
    // (whole workgroup: nothing of this tensor is its to update; chunk 0 always stays, it owns the tail)
    if ((long)blockIdx.x * blockDim.x * (vec ? 4 : 1) >= e.n) return;
    const int t = threadIdx.x;
    float A = a.A, B = a.B, bc1 = a.bc1, sbc2 = a.sbc2;
    if (a.sched_dev) {
        A = a.sched_dev[0];
        B = a.sched_dev[1];
        if constexpr (KIND == LEDN_OPTIM_ADAMW) {
            bc1 = a.sched_dev[2];
            sbc2 = a.sched_dev[3];
        }
    }
    OptimConsts c;
    c.gs = a.gscale;
    if constexpr (CLIP == OPT_CLIP_L2 || CLIP == OPT_CLIP_INF) {
        __shared__ float s_w[4];
        float tot = block256_combine<CLIP == OPT_CLIP_INF>(t < a.n_partials ? a.partials[t] : 0.f, s_w);
        if constexpr (CLIP == OPT_CLIP_L2) tot = sqrtf(tot);
        tot *= a.gscale;                                   // the norm of the gradient the update uses (DDP's mean)
        const float q = a.max_norm / (tot + 1e-6f);
        const float coef = q > 1.f ? 1.f : q;              // torch.clamp(max=1): a NaN coefficient stays NaN
        if (a.norm_out && blockIdx.x == 0 && blockIdx.y == 0 && t == 0) {
            a.norm_out[0] = tot;
            a.norm_out[1] = coef;
        }
        c.gs = a.gscale * coef;
    }
    c.cv = a.clip_value;
    c.lr = e.lr_mult * A + B;
    c.wd = e.wd_mult * a.weight_decay;
    c.mom = a.momentum;
    c.decay = 1.f - c.lr * c.wd;
    c.b1 = a.b1, c.omb1 = a.omb1, c.b2 = a.b2, c.omb2 = a.omb2;
    c.step = c.lr / bc1;
    c.sbc2 = sbc2;
    c.eps = a.eps;
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + t;
    if (vec) {
        const long nvec = e.n >> 2;
        float4* pv = reinterpret_cast<float4*>(e.p);
        float4* gv = reinterpret_cast<float4*>(e.g);
        float4* mv = reinterpret_cast<float4*>(e.m);
        float4* vv = reinterpret_cast<float4*>(e.v);
        for (long i = i0; i < nvec; i += stride) {
            float4 p = pv[i], m = mv[i], v = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 g = gv[i];
            if constexpr (KIND == LEDN_OPTIM_ADAMW) v = vv[i];
            optim_update<KIND, CLIP>(c, p.x, g.x, m.x, v.x);
            optim_update<KIND, CLIP>(c, p.y, g.y, m.y, v.y);
            optim_update<KIND, CLIP>(c, p.z, g.z, m.z, v.z);
            optim_update<KIND, CLIP>(c, p.w, g.w, m.w, v.w);
            mv[i] = m;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) vv[i] = v;
            pv[i] = p;
            gv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            {
                float4* av = reinterpret_cast<float4*>(avg);
                float4 x = p;
                if (!ema_copy) {
                    x = av[i];
                    x.x = ema_lerp(ema_w, x.x, p.x);
                    x.y = ema_lerp(ema_w, x.y, p.y);
                    x.z = ema_lerp(ema_w, x.z, p.z);
                    x.w = ema_lerp(ema_w, x.w, p.w);
                }
                av[i] = x;
            }
        }
        const long done = nvec << 2;
        if (blockIdx.x == 0 && done + t < e.n) {
            const long i = done + t;
            float p = e.p[i], m = e.m[i], v = 0.f;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) v = e.v[i];
            optim_update<KIND, CLIP>(c, p, e.g[i], m, v);
            e.m[i] = m;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) e.v[i] = v;
            e.p[i] = p;
            e.g[i] = 0.f;
            avg[i] = ema_copy ? p : ema_lerp(ema_w, avg[i], p);
        }
    } else {
        for (long i = i0; i < e.n; i += stride) {
            float p = e.p[i], m = e.m[i], v = 0.f;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) v = e.v[i];
            optim_update<KIND, CLIP>(c, p, e.g[i], m, v);
            e.m[i] = m;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) e.v[i] = v;
            e.p[i] = p;
            e.g[i] = 0.f;
            avg[i] = ema_copy ? p : ema_lerp(ema_w, avg[i], p);
        }
    }
}

// (every table entry of an AdamW step needs a second-moment pointer; the table lives on the device, so the caller says
// whether it filled them in: ledn_optim_desc.has_v)
// avgs == NULL: ledn_optim_step (optim_kernel); else ledn_optim_step_ema (optim_ema_kernel, same grid)
// the checks of an optimizer descriptor and its kernel arguments; *clip_out: the OPT_CLIP_* instance.  dev_bc: the bias
// corrections come from device memory (ledn_optim_step_guarded), the descriptor's are not looked at
static int optim_prepare(const ledn_optim_entry* table_dev, int n_tensors, long long max_n, const ledn_optim_desc* d,
                         bool dev_bc, OptimArgs* out, int* clip_out) {
    LEDN_REQUIRE(table_dev && d && n_tensors > 0 && max_n > 0);
    LEDN_REQUIRE(d->kind == LEDN_OPTIM_SGD || d->kind == LEDN_OPTIM_ADAMW);
    if (d->kind == LEDN_OPTIM_ADAMW) {
        LEDN_REQUIRE(d->has_v);
        LEDN_REQUIRE(d->beta1 >= 0.0 && d->beta1 < 1.0 && d->beta2 >= 0.0 && d->beta2 < 1.0 && d->eps > 0.f);
        LEDN_REQUIRE(dev_bc || d->sched_dev || (d->bc1 > 0.f && d->sqrt_bc2 > 0.f));
    }
    int clip = OPT_CLIP_OFF;
    if (d->clip == LEDN_CLIP_NORM) {
        LEDN_REQUIRE(d->norm_type == LEDN_NORM_L2 || d->norm_type == LEDN_NORM_INF);
        LEDN_REQUIRE(d->partials && d->n_partials >= 1 && d->n_partials <= LEDN_CLIP_MAX_PARTIALS && d->max_norm > 0.f);
        clip = d->norm_type == LEDN_NORM_L2 ? OPT_CLIP_L2 : OPT_CLIP_INF;
    } else if (d->clip == LEDN_CLIP_VALUE) {
        LEDN_REQUIRE(d->clip_value > 0.f);
        clip = OPT_CLIP_VALUE;
    } else {
        LEDN_REQUIRE(d->clip == LEDN_CLIP_OFF);
    }
    OptimArgs a;
    a.table = table_dev;
    a.sched_dev = d->sched_dev;
    a.A = d->lr_a, a.B = d->lr_b, a.bc1 = d->bc1, a.sbc2 = d->sqrt_bc2;
    a.momentum = d->momentum;
    a.b1 = (float)d->beta1, a.omb1 = (float)(1.0 - d->beta1);       // (torch: 1 - beta in double, then to the tensor's type)
    a.b2 = (float)d->beta2, a.omb2 = (float)(1.0 - d->beta2);
    a.eps = d->eps;
    a.weight_decay = d->weight_decay, a.gscale = d->grad_scale;
    a.partials = d->partials, a.n_partials = d->n_partials;
    a.max_norm = d->max_norm, a.clip_value = d->clip_value;
    a.norm_out = d->norm_out;
    *out = a;
    *clip_out = clip;
    return LEDN_OK;
}

// grid.x of the optimizer launches
static long optim_chunks(long long max_n) {
    const long chunks = cdiv(max_n, 256 * 8);
    return chunks > 64 ? 64 : chunks;
}

static int optim_launch(const ledn_optim_entry* table_dev, float* const* avgs, int n_tensors, long long max_n,
                        const ledn_optim_desc* d, float ema_w, const float* ema_w_dev, hipStream_t s) {
    OptimArgs a;
    int clip;
    const int rc = optim_prepare(table_dev, n_tensors, max_n, d, false, &a, &clip);
    if (rc != LEDN_OK) return rc;
    const dim3 grid((unsigned)optim_chunks(max_n), (unsigned)n_tensors);
#define LEDN_OPTIM(KIND, CLIP)                                                                                  \
    do {                                                                                                        \
        if (avgs) LEDN_LAUNCH((optim_ema_kernel<KIND, CLIP>), grid, dim3(256), 0, s, a, avgs, ema_w, ema_w_dev); \
        else LEDN_LAUNCH((optim_kernel<KIND, CLIP>), grid, dim3(256), 0, s, a);                                 \
    } while (0)
#define LEDN_OPTIM_KIND(KIND)                                        \
    switch (clip) {                                                  \
        case OPT_CLIP_L2: LEDN_OPTIM(KIND, OPT_CLIP_L2); break;      \
        case OPT_CLIP_INF: LEDN_OPTIM(KIND, OPT_CLIP_INF); break;    \
        case OPT_CLIP_VALUE: LEDN_OPTIM(KIND, OPT_CLIP_VALUE); break;\
        default: LEDN_OPTIM(KIND, OPT_CLIP_OFF); break;              \
    }
    if (d->kind == LEDN_OPTIM_SGD) { LEDN_OPTIM_KIND(LEDN_OPTIM_SGD) } else { LEDN_OPTIM_KIND(LEDN_OPTIM_ADAMW) }
#undef LEDN_OPTIM_KIND
#undef LEDN_OPTIM
    return check_launch();
}

int optim_step_impl(const ledn_optim_entry* table_dev, int n_tensors, long long max_n, const ledn_optim_desc* d,
                    hipStream_t s) {
    return optim_launch(table_dev, nullptr, n_tensors, max_n, d, 0.f, nullptr, s);
}

int optim_step_ema_impl(const ledn_optim_entry* table_dev, float* const* avg_table_dev, int n_tensors, long long max_n,
                        const ledn_optim_desc* d, float w, const float* w_dev, hipStream_t s) {
    LEDN_REQUIRE(avg_table_dev);
    LEDN_REQUIRE(w_dev || (w > 0.f && w <= 1.f));
    return optim_launch(table_dev, avg_table_dev, n_tensors, max_n, d, w, w_dev, s);
}

// ===========================================================================
// standalone multi-tensor weight averaging (ledn_ema_update): avg <- avg + w * (src - avg) over a table of {avg, src, n},
// for what the optimizer launch does not touch (frozen parameters, parameters without a gradient, BatchNorm running
// statistics).  grid, access rule, lerp and copy branch as optim_ema_kernel; no atomics, no reduction.
// ===========================================================================
__global__ void __launch_bounds__(256) ema_update_kernel(const ledn_ema_entry* table, float w_arg, const float* w_dev) {
    const ledn_ema_entry e = table[blockIdx.y];
    const bool vec = ((((uintptr_t)e.avg | (uintptr_t)e.src) & 15u) == 0) && e.n >= 4;
    if ((long)blockIdx.x * blockDim.x * (vec ? 4 : 1) >= e.n) return;
    const float w = w_dev ? *w_dev : w_arg;
    const bool copy = w >= 1.f;
    const int t = threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + t;
    if (vec) {
        const long nvec = e.n >> 2;
        float4* av = reinterpret_cast<float4*>(e.avg);
        const float4* sv = reinterpret_cast<const float4*>(e.src);
        for (long i = i0; i < nvec; i += stride) {
            const float4 p = sv[i];
            float4 x = p;
            if (!copy) {
                x = av[i];
                x.x = ema_lerp(w, x.x, p.x);
                x.y = ema_lerp(w, x.y, p.y);
                x.z = ema_lerp(w, x.z, p.z);
                x.w = ema_lerp(w, x.w, p.w);
            }
            av[i] = x;
        }
        const long i = (nvec << 2) + t;
        if (blockIdx.x == 0 && i < e.n) {
            const float p = e.src[i];
            e.avg[i] = copy ? p : ema_lerp(w, e.avg[i], p);
        }
    } else {
        for (long i = i0; i < e.n; i += stride) {
            const float p = e.src[i];
            e.avg[i] = copy ? p : ema_lerp(w, e.avg[i], p);
        }
    }
}

int ema_update_impl(const ledn_ema_entry* table_dev, int n_tensors, long long max_n, float w, const float* w_dev,
                    hipStream_t s) {
    LEDN_REQUIRE(table_dev && n_tensors > 0 && max_n > 0);
    LEDN_REQUIRE(w_dev || (w > 0.f && w <= 1.f));
    long chunks = cdiv(max_n, 256 * 8);
    if (chunks > 64) chunks = 64;
    LEDN_LAUNCH(ema_update_kernel, dim3((unsigned)chunks, (unsigned)n_tensors), dim3(256), 0, s, table_dev, w, w_dev);
    return check_launch();
}

// ===========================================================================
// step guard (ledn_grad_finite_pass, ledn_step_guard_verdict, ledn_optim_step_guarded): an optimizer step whose gradient
// holds an Inf or a NaN leaves parameters and optimizer state alone.  Three launches in stream order; the launch boundary
// is the only hand-off: the finite pass writes bad[] and one flag per workgroup, the one-workgroup verdict turns them into
// the persistent words {skip, counts, bias corrections, log mirrors, sticky record}, and the optimizer launch only READS
// those words -- no workgroup of it reads anything another workgroup of the same launch writes, so there is no ticket,
// no spin and no atomic anywhere.
// ===========================================================================
__device__ __forceinline__ unsigned nonfinite_bits(unsigned u) { return (u & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }
__device__ __forceinline__ unsigned nonfinite4(const uint4& v) {
    return nonfinite_bits(v.x) | nonfinite_bits(v.y) | nonfinite_bits(v.z) | nonfinite_bits(v.w);
}

// grid = (chunks, tensors) with few, long chunks (guard_chunks): most tensors of a network are small, every workgroup
// costs a table read, a barrier pair and a flag store whether it has elements or not, and the verdict reads every flag
// (the optimizer launch's 64 chunks per tensor would be 25472 workgroups and flag words for the shipped model).
// Per tensor: head = the 0-3 floats in front of the first 16-byte aligned address, then nvec 16-byte vectors (grid-stride over the chunks, four loads in flight per trip), then 0-3 tail
// floats; head and tail go to the first threads of chunk 0.  Every workgroup stores its own flag word; the ones that saw a
// bad element also store the same 1 to bad[tensor] (cleared by the memset node in front of the launch).
__global__ void __launch_bounds__(256) grad_finite_kernel(const ledn_optim_entry* table, int* bad, int* flags) {
    __shared__ int s_bad;
    const ledn_optim_entry e = table[blockIdx.y];
    const int t = threadIdx.x;
    const unsigned* g = reinterpret_cast<const unsigned*>(e.g);
    long head = (long)((16u - ((uintptr_t)g & 15u)) & 15u) >> 2;
    if (head > e.n) head = e.n;
    const long nvec = (e.n - head) >> 2;
    const int tail = (int)(e.n - head - (nvec << 2));
    const uint4* gv = reinterpret_cast<const uint4*>(g + head);
    const long stride = (long)gridDim.x * 256;
    unsigned acc = 0u;
    long v = (long)blockIdx.x * 256 + t;
    for (; v + 3 * stride < nvec; v += 4 * stride) {
        const uint4 a = gv[v], b = gv[v + stride], c = gv[v + 2 * stride], d = gv[v + 3 * stride];
        acc |= nonfinite4(a) | nonfinite4(b) | nonfinite4(c) | nonfinite4(d);
    }
    for (; v < nvec; v += stride) acc |= nonfinite4(gv[v]);
    if (blockIdx.x == 0) {
        if (t < head) acc |= nonfinite_bits(g[t]);
        if (t < tail) acc |= nonfinite_bits(g[head + (nvec << 2) + t]);
    }
    if (t == 0) s_bad = 0;
    __syncthreads();
    if (acc) s_bad = 1;                                     // (every writer stores the same value)
    __syncthreads();
    if (t == 0) {
        const int b = s_bad;
        flags[(long)blockIdx.y * gridDim.x + blockIdx.x] = b;
        if (b) bad[blockIdx.y] = 1;
    }
}

// grid.x of the finite pass = flag words per tensor: 4096 floats (four 16-byte loads per thread) per trip
static long guard_chunks(long long max_n) {
    const long chunks = cdiv(max_n, 4096);
    return chunks > LEDN_GUARD_MAX_CHUNKS ? LEDN_GUARD_MAX_CHUNKS : chunks;
}

static int guard_check(const ledn_optim_entry* table_dev, int n_tensors, long long max_n, const ledn_step_guard* gd) {
    LEDN_REQUIRE(table_dev && n_tensors > 0 && max_n > 0);
    LEDN_REQUIRE(gd && gd->words && gd->bad && gd->flags && gd->last_bad);
    LEDN_REQUIRE(((uintptr_t)gd->words & 7u) == 0);
    return LEDN_OK;
}

int grad_finite_pass_impl(const ledn_optim_entry* table_dev, int n_tensors, long long max_n, const ledn_step_guard* gd,
                          hipStream_t s) {
    const int rc = guard_check(table_dev, n_tensors, max_n, gd);
    if (rc != LEDN_OK) return rc;
    if (hipMemsetAsync(gd->bad, 0, sizeof(int) * (size_t)n_tensors, s) != hipSuccess) return LEDN_ELAUNCH;
    LEDN_LAUNCH(grad_finite_kernel, dim3((unsigned)guard_chunks(max_n), (unsigned)n_tensors), dim3(256), 0, s, table_dev,
                gd->bad, gd->flags);
    return check_launch();
}

// one workgroup.  Thread 0 alone touches the words; the sticky copy of bad[] is spread over the threads.
__global__ void __launch_bounds__(256) step_guard_verdict_kernel(ledn_guard_words* w, const int* bad, const int* flags,
                                                                 int* last_bad, int n_tensors, long n_flags, double beta1,
                                                                 double beta2, long long iter, const long long* iter_dev) {
    __shared__ int s_bad;
    const int t = threadIdx.x;
    int acc = 0;
    for (long i = t; i < n_flags; i += 256) acc |= flags[i];
    if (t == 0) s_bad = 0;
    __syncthreads();
    if (acc) s_bad = 1;
    __syncthreads();
    const int skip = s_bad;
    if (skip)
        for (int i = t; i < n_tensors; i += 256) last_bad[i] = bad[i];
    if (t == 0) {
        const long long applied = w->applied, skipped = w->skipped + (skip ? 1 : 0);
        const double tt = (double)(applied + 1);            // the step count an applied step has (torch: 1-based)
        w->bc1 = (float)(1.0 - pow(beta1, tt));
        w->sqrt_bc2 = (float)sqrt(1.0 - pow(beta2, tt));
        w->skip = skip;
        w->applied = applied + (skip ? 0 : 1);
        w->skipped = skipped;
        w->grad_finite = skip ? 0.f : 1.f;
        w->skipped_steps = (float)skipped;
        if (skip) {
            w->has_last = 1;
            w->last_iter = iter_dev ? *iter_dev : iter;
        }
    }
}

int step_guard_verdict_impl(const ledn_optim_entry* table_dev, int n_tensors, long long max_n, const ledn_step_guard* gd,
                            double beta1, double beta2, long long iter, const long long* iter_dev, hipStream_t s) {
    const int rc = guard_check(table_dev, n_tensors, max_n, gd);
    if (rc != LEDN_OK) return rc;
    LEDN_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
    LEDN_REQUIRE(!iter_dev || ((uintptr_t)iter_dev & 7u) == 0);
    LEDN_LAUNCH(step_guard_verdict_kernel, dim3(1), dim3(256), 0, s, gd->words, gd->bad, gd->flags, gd->last_bad, n_tensors,
                guard_chunks(max_n) * (long)n_tensors, beta1, beta2, iter, iter_dev);
    return check_launch();
}

// the averaged copy of a step that is left out: avg + w * (p - avg) with every operation rounded on its own, so that the
// same f32 expression in torch gives its bits on the device too (ema_lerp's fused form is the applied step's)
__device__ __forceinline__ float ema_lerp_skip(float w, float avg, float p) { return opt_add(avg, opt_mul(w, opt_add(p, -avg))); }

// optim_ema_kernel with the skip predicate and the bias corrections of the guard words; EMA = false is optim_kernel's
// column set (avgs == NULL).  A kernel of its own for the reason optim_ema_kernel is one: the existing launches keep
// their code.  Everything between the skip branch and the end is optim_ema_kernel's text, so an applied step has its bits.
template <int KIND, int CLIP, bool EMA>
__global__ void __launch_bounds__(256) optim_guarded_kernel(const OptimArgs a, float* const* avgs, float w_arg, const float* w_dev,
                                                            const ledn_guard_words* gw) {
    const ledn_optim_entry e = a.table[blockIdx.y];
    float* avg = nullptr;
    float ema_w = 1.f;
    if constexpr (EMA) {
        avg = avgs[blockIdx.y];
        ema_w = w_dev ? *w_dev : w_arg;
    }
    const bool vec = ((((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v | (uintptr_t)avg) & 15u) == 0) && e.n >= 4;
    const bool ema_copy = ema_w >= 1.f;                    // (the same in every thread of the grid)
    // (whole workgroup: nothing of this tensor is its to update; chunk 0 always stays, it owns the tail)
    if ((long)blockIdx.x * blockDim.x * (vec ? 4 : 1) >= e.n) return;
    const int t = threadIdx.x;
    const int skip = gw->skip;                             // (one word, the same in every workgroup: the verdict launch wrote it)
    float A = a.A, B = a.B, bc1 = 1.f, sbc2 = 1.f;
    if (a.sched_dev) {
        A = a.sched_dev[0];
        B = a.sched_dev[1];
    }
    if constexpr (KIND == LEDN_OPTIM_ADAMW) {
        bc1 = gw->bc1;
        sbc2 = gw->sqrt_bc2;
    }
    OptimConsts c;
    c.gs = a.gscale;
    if constexpr (CLIP == OPT_CLIP_L2 || CLIP == OPT_CLIP_INF) {
        __shared__ float s_w[4];
        float tot = block256_combine<CLIP == OPT_CLIP_INF>(t < a.n_partials ? a.partials[t] : 0.f, s_w);
        if constexpr (CLIP == OPT_CLIP_L2) tot = sqrtf(tot);
        tot *= a.gscale;                                   // the norm of the gradient the update uses (DDP's mean)
        const float q = a.max_norm / (tot + 1e-6f);
        const float coef = q > 1.f ? 1.f : q;              // torch.clamp(max=1): a NaN coefficient stays NaN
        if (a.norm_out && blockIdx.x == 0 && blockIdx.y == 0 && t == 0) {
            a.norm_out[0] = tot;
            a.norm_out[1] = coef;
        }
        c.gs = a.gscale * coef;
    }
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = (long)blockIdx.x * blockDim.x + t;
    if (skip) {
        // the step is left out: only the gradient is cleared and the averaged copy follows the unchanged p
        if (vec) {
            const long nvec = e.n >> 2;
            float4* gv = reinterpret_cast<float4*>(e.g);
            for (long i = i0; i < nvec; i += stride) {
                gv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (EMA) {
                    float4* av = reinterpret_cast<float4*>(avg);
                    const float4 p = reinterpret_cast<const float4*>(e.p)[i];
                    float4 x = p;
                    if (!ema_copy) {
                        x = av[i];
                        x.x = ema_lerp_skip(ema_w, x.x, p.x);
                        x.y = ema_lerp_skip(ema_w, x.y, p.y);
                        x.z = ema_lerp_skip(ema_w, x.z, p.z);
                        x.w = ema_lerp_skip(ema_w, x.w, p.w);
                    }
                    av[i] = x;
                }
            }
            const long i = (nvec << 2) + t;
            if (blockIdx.x == 0 && i < e.n) {
                e.g[i] = 0.f;
                if constexpr (EMA) avg[i] = ema_copy ? e.p[i] : ema_lerp_skip(ema_w, avg[i], e.p[i]);
            }
        } else {
            for (long i = i0; i < e.n; i += stride) {
                e.g[i] = 0.f;
                if constexpr (EMA) avg[i] = ema_copy ? e.p[i] : ema_lerp_skip(ema_w, avg[i], e.p[i]);
            }
        }
        return;
    }
    c.cv = a.clip_value;
    c.lr = e.lr_mult * A + B;
    c.wd = e.wd_mult * a.weight_decay;
    c.mom = a.momentum;
    c.decay = 1.f - c.lr * c.wd;
    c.b1 = a.b1, c.omb1 = a.omb1, c.b2 = a.b2, c.omb2 = a.omb2;
    c.step = c.lr / bc1;
    c.sbc2 = sbc2;
    c.eps = a.eps;
    if (vec) {
        const long nvec = e.n >> 2;
        float4* pv = reinterpret_cast<float4*>(e.p);
        float4* gv = reinterpret_cast<float4*>(e.g);
        float4* mv = reinterpret_cast<float4*>(e.m);
        float4* vv = reinterpret_cast<float4*>(e.v);
        for (long i = i0; i < nvec; i += stride) {
            float4 p = pv[i], m = mv[i], v = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 g = gv[i];
            if constexpr (KIND == LEDN_OPTIM_ADAMW) v = vv[i];
            optim_update<KIND, CLIP>(c, p.x, g.x, m.x, v.x);
            optim_update<KIND, CLIP>(c, p.y, g.y, m.y, v.y);
            optim_update<KIND, CLIP>(c, p.z, g.z, m.z, v.z);
            optim_update<KIND, CLIP>(c, p.w, g.w, m.w, v.w);
            mv[i] = m;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) vv[i] = v;
            pv[i] = p;
            gv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (EMA) {
                float4* av = reinterpret_cast<float4*>(avg);
                float4 x = p;
                if (!ema_copy) {
                    x = av[i];
                    x.x = ema_lerp(ema_w, x.x, p.x);
                    x.y = ema_lerp(ema_w, x.y, p.y);
                    x.z = ema_lerp(ema_w, x.z, p.z);
                    x.w = ema_lerp(ema_w, x.w, p.w);
                }
                av[i] = x;
            }
        }
        const long done = nvec << 2;
        if (blockIdx.x == 0 && done + t < e.n) {
            const long i = done + t;
            float p = e.p[i], m = e.m[i], v = 0.f;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) v = e.v[i];
            optim_update<KIND, CLIP>(c, p, e.g[i], m, v);
            e.m[i] = m;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) e.v[i] = v;
            e.p[i] = p;
            e.g[i] = 0.f;
            if constexpr (EMA) avg[i] = ema_copy ? p : ema_lerp(ema_w, avg[i], p);
        }
    } else {
        for (long i = i0; i < e.n; i += stride) {
            float p = e.p[i], m = e.m[i], v = 0.f;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) v = e.v[i];
            optim_update<KIND, CLIP>(c, p, e.g[i], m, v);
            e.m[i] = m;
            if constexpr (KIND == LEDN_OPTIM_ADAMW) e.v[i] = v;
            e.p[i] = p;
            e.g[i] = 0.f;
            if constexpr (EMA) avg[i] = ema_copy ? p : ema_lerp(ema_w, avg[i], p);
        }
    }
}

int optim_step_guarded_impl(const ledn_optim_entry* table_dev, float* const* avgs, int n_tensors, long long max_n,
                            const ledn_optim_desc* d, const ledn_step_guard* gd, float w, const float* w_dev, hipStream_t s) {
    OptimArgs a;
    int clip;
    int rc = optim_prepare(table_dev, n_tensors, max_n, d, true, &a, &clip);
    if (rc != LEDN_OK) return rc;
    rc = guard_check(table_dev, n_tensors, max_n, gd);
    if (rc != LEDN_OK) return rc;
    LEDN_REQUIRE(!avgs || w_dev || (w > 0.f && w <= 1.f));
    const dim3 grid((unsigned)optim_chunks(max_n), (unsigned)n_tensors);
    const ledn_guard_words* gw = gd->words;
#define LEDN_OPTIM(KIND, CLIP)                                                                                              \
    do {                                                                                                                    \
        if (avgs) LEDN_LAUNCH((optim_guarded_kernel<KIND, CLIP, true>), grid, dim3(256), 0, s, a, avgs, w, w_dev, gw);     \
        else LEDN_LAUNCH((optim_guarded_kernel<KIND, CLIP, false>), grid, dim3(256), 0, s, a, avgs, w, w_dev, gw);         \
    } while (0)
#define LEDN_OPTIM_KIND(KIND)                                        \
    switch (clip) {                                                  \
        case OPT_CLIP_L2: LEDN_OPTIM(KIND, OPT_CLIP_L2); break;      \
        case OPT_CLIP_INF: LEDN_OPTIM(KIND, OPT_CLIP_INF); break;    \
        case OPT_CLIP_VALUE: LEDN_OPTIM(KIND, OPT_CLIP_VALUE); break;\
        default: LEDN_OPTIM(KIND, OPT_CLIP_OFF); break;              \
    }
    if (d->kind == LEDN_OPTIM_SGD) { LEDN_OPTIM_KIND(LEDN_OPTIM_SGD) } else { LEDN_OPTIM_KIND(LEDN_OPTIM_ADAMW) }
#undef LEDN_OPTIM_KIND
#undef LEDN_OPTIM
    return check_launch();
}

}  // namespace ledn
