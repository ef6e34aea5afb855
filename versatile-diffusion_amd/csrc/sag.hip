// Self-attention guidance (Hong et al., ICCV 2023) on gfx950: the three launches it adds to a step.  Contracts (operands, the
// written-out roundings): include/vd_hip.h.
//
// vd_sag_mass_f16: the column mass of a self-attention map, mass[b, j] = (1 / H) sum_h sum_i softmax_j(scale q_i . k_j).  The
// attention kernels are online-softmax and never hold the map, so this entry forms the scores a second time, in fp32 and without
// rounding P.  One block per sample walks the heads in order: pass 1 keeps the row maximum and the row sum of every query in LDS,
// pass 2 forms the scores again tile by tile and sums the probabilities per key (a map of at most 64 tokens is one tile: its
// scores are formed once and stay in registers for both passes).  Every sum has a fixed order (registers, one
// 16-lane butterfly, LDS partials added in ascending order): no float atomics, the result is bit-identical run to run.  The
// scores are plain dot products on the vector pipe (v_dot2_f32_f16): at the sizes of the middle block (N = 64 .. 144, 8 heads of
// 160) that is 2 x 10 MFLOP per sample, measured by tools/probes/sag_step_time.py.
//
// vd_sag_degrade_f16: ratio-combined mass -> threshold -> nearest-neighbour mask on the latent grid -> 9 x 9 separable Gaussian
// blur of the step's data prediction where the mask is set -> re-noised latent, in one launch.  A 32 x 32 tile of one plane per
// block; p0 of the tile and its 4-pixel halo (reflected at the plane's edges) is staged in LDS; a tile without a masked pixel
// skips the blur.
//
// vd_sag_fold_f16: folds the degraded prediction into replica 0 of the step's eps batch (vd_pag_fold_f16's scheme), so that every
// fused update and the rescale-factor kernel run unchanged.
#include <math.h>

#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

constexpr int SAG_THREADS = 256;

// fp32 -> fp16 as a rounding of its own (pag.hip's rule): the empty asm keeps the fp32 value, so the conversion is not folded into
// the fma in front of it.
__device__ __forceinline__ f16 sag_round_f16(float v) {
    asm("" : "+v"(v));
    return (f16)v;
}

// ---- mass ------------------------------------------------------------------------------------------------------------------------
constexpr int MT = 64;            // queries and keys per score tile: 256 threads x (4 x 4) scores
constexpr int MDC = 160;          // head-dim columns staged per chunk: the widest UNet head in one piece
constexpr int MPRE = MT * (MDC / 8) / SAG_THREADS;      // 16-byte pieces of one staged tile per thread
constexpr int MRS = MDC / 2 + 1;  // LDS row stride in dwords (odd: the 16 key rows a wave reads fall into 16 banks)
constexpr int MASS_MAX_N = 1024;

// rows row0 .. row0 + 63 (zero past N), columns d0 .. d0 + dc - 1 of one head, 16 bytes per access, into dst[64][MRS]
__device__ __forceinline__ void mass_stage(const f16* src, int ld, int row0, int N, int d0, int dc, uint32_t* dst) {
    const int chunks = dc / 8;
    for (int t = threadIdx.x; t < MT * chunks; t += SAG_THREADS) {
        const int r = t / chunks, c = t - r * chunks;
        uint4 u = make_uint4(0u, 0u, 0u, 0u);
        if (row0 + r < N) u = *reinterpret_cast<const uint4*>(src + (int64_t)(row0 + r) * ld + d0 + c * 8);
        uint32_t* p = dst + r * MRS + c * 4;
        p[0] = u.x; p[1] = u.y; p[2] = u.z; p[3] = u.w;
    }
}

// the same tile (dc = D <= MDC) through registers: the loads of the next head are in flight while this head's scores are formed
__device__ __forceinline__ void mass_fetch(const f16* src, int ld, int N, int D, uint4 (&r)[MPRE]) {
    const int chunks = D / 8;
#pragma unroll
    for (int i = 0; i < MPRE; ++i) {
        const int t = threadIdx.x + i * SAG_THREADS;
        const int row = t / chunks, c = t - row * chunks;
        r[i] = make_uint4(0u, 0u, 0u, 0u);
        if (t < MT * chunks && row < N) r[i] = *reinterpret_cast<const uint4*>(src + (int64_t)row * ld + c * 8);
    }
}
__device__ __forceinline__ void mass_put(const uint4 (&r)[MPRE], int D, uint32_t* dst) {
    const int chunks = D / 8;
#pragma unroll
    for (int i = 0; i < MPRE; ++i) {
        const int t = threadIdx.x + i * SAG_THREADS;
        if (t < MT * chunks) {
            const int row = t / chunks, c = t - row * chunks;
            uint32_t* p = dst + row * MRS + c * 4;
            p[0] = r[i].x; p[1] = r[i].y; p[2] = r[i].z; p[3] = r[i].w;
        }
    }
}

// acc[a][c] += q[ty + 16 a] . k[tx + 16 c] over the staged dc columns, ascending
__device__ __forceinline__ void mass_dot(const uint32_t* qs, const uint32_t* ks, int ty, int tx, int dc, float (&acc)[4][4]) {
    for (int dd = 0; dd < dc / 2; ++dd) {
        f16x2 qv[4], kv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) qv[a] = __builtin_bit_cast(f16x2, qs[(ty + 16 * a) * MRS + dd]);
#pragma unroll
        for (int c = 0; c < 4; ++c) kv[c] = __builtin_bit_cast(f16x2, ks[(tx + 16 * c) * MRS + dd]);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[a][c] = __builtin_amdgcn_fdot2(qv[a], kv[c], acc[a][c], false);
    }
}

__device__ __forceinline__ void mass_scores(const f16* qh, const f16* kh, int ldq, int ldk, int q0, int k0, int N, int D, uint32_t* qs,
                                            uint32_t* ks, int ty, int tx, float (&acc)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
    for (int d0 = 0; d0 < D; d0 += MDC) {
        const int dc = min(MDC, D - d0);
        __syncthreads();        // the previous chunk's (tile's) reads are done
        mass_stage(qh, ldq, q0, N, d0, dc, qs);
        mass_stage(kh, ldk, k0, N, d0, dc, ks);
        __syncthreads();
        mass_dot(qs, ks, ty, tx, dc, acc);
    }
}

__global__ __launch_bounds__(SAG_THREADS) void sag_mass_kernel(const f16* q, const f16* k, float* mass, int H, int N, int D, int ldq,
                                                               int ldk, int64_t sq, int64_t sk, float scale) {
    __shared__ uint32_t qs[MT * MRS];
    __shared__ uint32_t ks[MT * MRS];
    __shared__ float rowm[MASS_MAX_N];
    __shared__ float rowil[MASS_MAX_N];
    __shared__ float colsum[MASS_MAX_N];
    __shared__ float part[16][MT];
    const int b = blockIdx.x;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int tiles = (N + MT - 1) / MT;
    for (int j = threadIdx.x; j < N; j += SAG_THREADS) colsum[j] = 0.f;
    if (tiles == 1 && D <= MDC) {
        // one tile holds the whole map of a head (the middle block up to 512 x 512 pixels): the scores are formed once and stay in
        // registers for both passes; q and k of the next head are fetched while this head computes
        uint4 rq[MPRE], rk[MPRE];
        mass_fetch(q + (int64_t)b * sq, ldq, N, D, rq);
        mass_fetch(k + (int64_t)b * sk, ldk, N, D, rk);
        for (int h = 0; h < H; ++h) {
            __syncthreads();        // the previous head's reads of the tiles and of part[] are done
            mass_put(rq, D, qs);
            mass_put(rk, D, ks);
            if (h + 1 < H) {
                mass_fetch(q + (int64_t)b * sq + (int64_t)(h + 1) * D, ldq, N, D, rq);
                mass_fetch(k + (int64_t)b * sk + (int64_t)(h + 1) * D, ldk, N, D, rk);
            }
            __syncthreads();
            float acc[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
            mass_dot(qs, ks, ty, tx, D, acc);
            float col[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                float e[4], m = -INFINITY, l = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    e[c] = (tx + 16 * c < N) ? scale * acc[a][c] : -INFINITY;
                    m = fmaxf(m, e[c]);
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    e[c] = expf(e[c] - m);
                    l += e[c];
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) l += __shfl_xor(l, o, 64);
                if (ty + 16 * a < N) {
                    const float il = 1.0f / l;
#pragma unroll
                    for (int c = 0; c < 4; ++c) col[c] += e[c] * il;
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) part[ty][tx + 16 * c] = col[c];
            __syncthreads();
            if (threadIdx.x < N) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) s += part[r][threadIdx.x];
                colsum[threadIdx.x] += s;
            }
        }
        __syncthreads();
        const float inv_h1 = 1.0f / (float)H;
        for (int j = threadIdx.x; j < N; j += SAG_THREADS) mass[(int64_t)b * N + j] = colsum[j] * inv_h1;
        return;
    }
    for (int h = 0; h < H; ++h) {
        const f16* qh = q + (int64_t)b * sq + (int64_t)h * D;
        const f16* kh = k + (int64_t)b * sk + (int64_t)h * D;
        // pass 1: row maximum and row sum of every query
        for (int qt = 0; qt < tiles; ++qt) {
            float m[4], l[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { m[a] = -INFINITY; l[a] = 0.f; }
            for (int kt = 0; kt < tiles; ++kt) {
                float acc[4][4];
                mass_scores(qh, kh, ldq, ldk, qt * MT, kt * MT, N, D, qs, ks, ty, tx, acc);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    float s[4], tm = -INFINITY;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        s[c] = (kt * MT + tx + 16 * c < N) ? scale * acc[a][c] : -INFINITY;
                        tm = fmaxf(tm, s[c]);
                    }
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) tm = fmaxf(tm, __shfl_xor(tm, o, 64));
                    const float mn = fmaxf(m[a], tm);       // finite: tile 0 holds key 0
                    float ts = 0.f;
#pragma unroll
                    for (int c = 0; c < 4; ++c) ts += expf(s[c] - mn);
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) ts += __shfl_xor(ts, o, 64);
                    l[a] = l[a] * expf(m[a] - mn) + ts;
                    m[a] = mn;
                }
            }
            if (tx == 0) {
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const int i = qt * MT + ty + 16 * a;
                    if (i < N) { rowm[i] = m[a]; rowil[i] = 1.0f / l[a]; }
                }
            }
        }
        __syncthreads();
        // pass 2: the scores again, summed per key over the queries
        for (int kt = 0; kt < tiles; ++kt) {
            float col[4] = {0.f, 0.f, 0.f, 0.f};
            for (int qt = 0; qt < tiles; ++qt) {
                float acc[4][4];
                mass_scores(qh, kh, ldq, ldk, qt * MT, kt * MT, N, D, qs, ks, ty, tx, acc);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const int i = qt * MT + ty + 16 * a;
                    if (i < N) {
                        const float mi = rowm[i], il = rowil[i];
#pragma unroll
                        for (int c = 0; c < 4; ++c) col[c] += expf(scale * acc[a][c] - mi) * il;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) part[ty][tx + 16 * c] = col[c];
            __syncthreads();
            if (threadIdx.x < MT) {
                const int j = kt * MT + threadIdx.x;
                if (j < N) {
                    float s = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) s += part[r][threadIdx.x];
                    colsum[j] += s;
                }
            }
            __syncthreads();
        }
    }
    const float inv_h = 1.0f / (float)H;
    for (int j = threadIdx.x; j < N; j += SAG_THREADS) mass[(int64_t)b * N + j] = colsum[j] * inv_h;
}

// ---- degrade ---------------------------------------------------------------------------------------------------------------------
constexpr int DT = 32;            // tile side
constexpr int DR = 4;             // blur radius: nine taps
constexpr int DP = DT + 2 * DR;   // staged side

// torch's "reflect" padding (no edge repeat); indices further out than the halo of a valid pixel are clamped (their values are not used)
__device__ __forceinline__ int sag_refl(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(SAG_THREADS) void sag_degrade_kernel(const f16* x, const f16* eps, const float* mass, const float* ratio, int T,
                                                                  const float* taps, const float* coef, f16* xd, int B, int C, int H,
                                                                  int W, int Hm, int Wm, int tiles_x) {
    __shared__ float p0s[DP][DP + 1];
    __shared__ float rps[DP][DT + 1];
    const int ty0 = (blockIdx.x / tiles_x) * DT, tx0 = (blockIdx.x % tiles_x) * DT;
    const int c = blockIdx.y, b = blockIdx.z;
    const int64_t plane = ((int64_t)b * C + c) * H * W;
    const f16* xp = x + plane;
    const f16* ep = eps + plane;
    f16* op = xd + plane;
    const float sa = coef[0], s1 = coef[1], isa = coef[2];
    const int Nm = Hm * Wm;
    // the mask of this thread's four pixels: m = fma(r_t, mass_t, m), t ascending from 0;  masked <=> m > 1
    bool masked[4];
    int any = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = threadIdx.x + u * SAG_THREADS;
        const int y = ty0 + t / DT, xx = tx0 + t % DT;
        masked[u] = false;
        if (y < H && xx < W) {
            const int j = (int)(((int64_t)y * Hm) / H) * Wm + (int)(((int64_t)xx * Wm) / W);
            float m = 0.f;
            for (int tt = 0; tt < T; ++tt) m = fmaf(ratio[tt], mass[((int64_t)tt * B + b) * Nm + j], m);
            masked[u] = m > 1.0f;
            any |= masked[u] ? 1 : 0;
        }
    }
    any = __syncthreads_or(any);
    if (!any) {     // d = p0 everywhere: no staging, no blur
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = threadIdx.x + u * SAG_THREADS;
            const int y = ty0 + t / DT, xx = tx0 + t % DT;
            if (y < H && xx < W) {
                const int64_t o = (int64_t)y * W + xx;
                const float e = (float)ep[o];
                const float p0 = fmaf(-s1, e, (float)xp[o]) * isa;
                op[o] = sag_round_f16(fmaf(sa, p0, s1 * e));
            }
        }
        return;
    }
    float g[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) g[i] = taps[i];
    for (int t = threadIdx.x; t < DP * DP; t += SAG_THREADS) {
        const int r = t / DP, cc = t - r * DP;
        const int64_t o = (int64_t)sag_refl(ty0 + r - DR, H) * W + sag_refl(tx0 + cc - DR, W);
        p0s[r][cc] = fmaf(-s1, (float)ep[o], (float)xp[o]) * isa;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < DP * DT; t += SAG_THREADS) {      // the row pass: along x, on every staged row
        const int r = t / DT, cc = t - r * DT;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 9; ++j) acc = fmaf(g[j], p0s[r][cc + j], acc);
        rps[r][cc] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int t = threadIdx.x + u * SAG_THREADS;
        const int ly = t / DT, lx = t % DT;
        const int y = ty0 + ly, xx = tx0 + lx;
        if (y < H && xx < W) {
            float d = p0s[ly + DR][lx + DR];
            if (masked[u]) {
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < 9; ++i) acc = fmaf(g[i], rps[ly + i][lx], acc);
                d = acc;
            }
            const int64_t o = (int64_t)y * W + xx;
            op[o] = sag_round_f16(fmaf(sa, d, s1 * (float)ep[o]));
        }
    }
}

// ---- fold ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f16 sag_fold_one(f16 a, f16 d, float w) {
    const float af = (float)a;
    return sag_round_f16(fmaf(w, af - (float)d, af));
}

template <bool VEC>
__global__ __launch_bounds__(SAG_THREADS) void sag_fold_kernel(f16* eps, const f16* ed, int64_t n, const float* wp) {
    const float w = *wp;
    if (w == 0.f) return;       // nothing to fold: replica 0 keeps its bits (a -0 and a NaN payload included)
    const size_t stride = (size_t)gridDim.x * SAG_THREADS;
    const size_t work = VEC ? (size_t)(n / 8) : (size_t)n;
    for (size_t t = (size_t)blockIdx.x * SAG_THREADS + threadIdx.x; t < work; t += stride) {
        if constexpr (VEC) {
            U4H8 va, vd;
            va.u = *reinterpret_cast<const uint4*>(eps + t * 8);
            vd.u = *reinterpret_cast<const uint4*>(ed + t * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) va.e[j] = sag_fold_one(va.e[j], vd.e[j], w);
            *reinterpret_cast<uint4*>(eps + t * 8) = va.u;
        } else {
            eps[t] = sag_fold_one(eps[t], ed[t], w);
        }
    }
}

}  // namespace

extern "C" int vd_sag_mass_f16(const void* q, const void* k, float* mass, int B, int H, int N, int D, int ldq, int ldk, int64_t sq,
                               int64_t sk, float scale, hipStream_t stream) {
    VD_REQUIRE(q && k && mass, "vd_sag_mass_f16: null pointer");
    VD_REQUIRE(B > 0 && H > 0 && N > 0 && D > 0, "vd_sag_mass_f16: empty problem B=%d H=%d N=%d D=%d", B, H, N, D);
    VD_REQUIRE(N <= MASS_MAX_N, "vd_sag_mass_f16: N = %d tokens, at most %d (the row statistics of a head live in LDS)", N, MASS_MAX_N);
    const bool wide = H == 1 && (D == 128 || D == 256 || D == 512);
    VD_REQUIRE(D == 40 || D == 64 || D == 80 || D == 160 || wide,
               "vd_sag_mass_f16: unsupported head dim %d (supported: 40, 64, 80, 160; one head of 128 / 256 / 512)", D);
    VD_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && sq % 8 == 0 && sk % 8 == 0 && vd_aligned16(q) && vd_aligned16(k),
               "vd_sag_mass_f16: q and k must be 16-byte aligned with leading dimensions and sample strides that are multiples of 8");
    VD_REQUIRE(ldq >= (int64_t)H * D && ldk >= (int64_t)H * D, "vd_sag_mass_f16: ldq = %d and ldk = %d must cover the H * D = %lld columns",
               ldq, ldk, (long long)H * D);
    VD_REQUIRE(((uintptr_t)mass & 3) == 0, "vd_sag_mass_f16: mass must be aligned to its element size");
    hipLaunchKernelGGL(sag_mass_kernel, dim3(B), dim3(SAG_THREADS), 0, stream, (const f16*)q, (const f16*)k, mass, H, N, D, ldq, ldk, sq, sk,
                       scale);
    return vd_check_launch("vd_sag_mass_f16");
}

extern "C" int vd_sag_degrade_f16(const void* x, const void* eps0, const float* mass, const float* ratio, int T, const float* taps,
                                  const float* coef, void* xd, int B, int C, int H, int W, int Hm, int Wm, hipStream_t stream) {
    VD_REQUIRE(x && eps0 && mass && ratio && taps && coef && xd, "vd_sag_degrade_f16: null pointer");
    VD_REQUIRE(B > 0 && C > 0 && T > 0 && Hm > 0 && Wm > 0, "vd_sag_degrade_f16: empty problem B=%d C=%d T=%d Hm=%d Wm=%d", B, C, T, Hm, Wm);
    VD_REQUIRE(H >= 5 && W >= 5, "vd_sag_degrade_f16: the plane is %d x %d, the reflected 9-tap blur needs H, W >= 5", H, W);
    VD_REQUIRE(C <= 65535 && B <= 65535, "vd_sag_degrade_f16: B = %d and C = %d must stay below 65536", B, C);
    VD_REQUIRE((int64_t)Hm * Wm < (1ll << 31) && (int64_t)H * W < (1ll << 31), "vd_sag_degrade_f16: the grids are too large");
    VD_REQUIRE(((uintptr_t)x & 1) == 0 && ((uintptr_t)eps0 & 1) == 0 && ((uintptr_t)xd & 1) == 0 && ((uintptr_t)mass & 3) == 0 &&
                   ((uintptr_t)ratio & 3) == 0 && ((uintptr_t)taps & 3) == 0 && ((uintptr_t)coef & 3) == 0,
               "vd_sag_degrade_f16: operands must be aligned to their element size");
    const int tiles_x = (W + DT - 1) / DT, tiles_y = (H + DT - 1) / DT;
    VD_REQUIRE((int64_t)tiles_x * tiles_y < (1ll << 31), "vd_sag_degrade_f16: too many tiles");
    hipLaunchKernelGGL(sag_degrade_kernel, dim3(tiles_x * tiles_y, C, B), dim3(SAG_THREADS), 0, stream, (const f16*)x, (const f16*)eps0, mass,
                       ratio, T, taps, coef, (f16*)xd, B, C, H, W, Hm, Wm, tiles_x);
    return vd_check_launch("vd_sag_degrade_f16");
}

extern "C" int vd_sag_fold_f16(void* eps, const void* e_d, int64_t n, const float* w, hipStream_t stream) {
    VD_REQUIRE(eps && e_d && w, "vd_sag_fold_f16: null pointer");
    VD_REQUIRE(n > 0, "vd_sag_fold_f16: n = %lld must be positive", (long long)n);
    VD_REQUIRE(((uintptr_t)eps & 1) == 0 && ((uintptr_t)e_d & 1) == 0 && ((uintptr_t)w & 3) == 0,
               "vd_sag_fold_f16: eps, e_d and w must be aligned to their element size");
    if (vd_aligned16(eps) && vd_aligned16(e_d) && n % 8 == 0) {
        hipLaunchKernelGGL(sag_fold_kernel<true>, dim3(grid_for((size_t)(n / 8), SAG_THREADS, 2048)), dim3(SAG_THREADS), 0, stream, (f16*)eps,
                           (const f16*)e_d, n, w);
    } else {
        hipLaunchKernelGGL(sag_fold_kernel<false>, dim3(grid_for((size_t)n, SAG_THREADS, 2048)), dim3(SAG_THREADS), 0, stream, (f16*)eps,
                           (const f16*)e_d, n, w);
    }
    return vd_check_launch("vd_sag_fold_f16");
}
