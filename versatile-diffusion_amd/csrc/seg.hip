// Smoothed energy guidance (Hong, "Smoothed Energy Guidance: Guiding Diffusion Models with Reduced Energy Curvature of Attention",
// NeurIPS 2024) on gfx950: the one pass it adds to a step.  Contract (operands, the written-out roundings): include/vd_hip.h.
//
// vd_attention_qblur_f16: self-attention whose QUERIES are Gaussian-blurred over the (gh, gw) token grid for the samples from
// `blur_from` on.  The samples in front of it go through vd_attention_f16 itself (the same kernel instances on a smaller batch: a
// sample's bits do not depend on the batch it sits in); for the others ONE launch writes the blurred queries into the caller's
// workspace qb and vd_attention_f16 runs with qb as its query.
//
// The blur is separable: a block takes a band of grid rows x one group of 8-channel chunks of one sample, writes the horizontal
// pass of every grid row its band reads (the reflected hull of the band) as fp32 into LDS, and runs the vertical pass from there.
// A lane's horizontal chain reads q straight from memory: the 2R + 1 taps of a row come back from L1.  Where the hull does not fit
// in LDS (a wide grid with a large R) the direct kernel recomputes the horizontal chain per vertical tap in registers: the same
// fp32 operations in the same order, so the same bits.  R = -1 (sigma = infinity): every query becomes the sample's mean query --
// one block per (sample, 8 channels), per-thread sums over tokens t, t + 256, ... ascending, then a fixed tree over the block.
#include <stdio.h>

#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_LDS_BYTES = 48 * 1024;     // per block, so that several blocks share a CU
constexpr int SEG_BAND = 8;                  // grid rows per block at most

// fp32 -> fp16 as a rounding of its own (pag.hip's rule): the empty asm keeps the fp32 value out of a fused mix-fma
__device__ __forceinline__ f16 seg_round_f16(float v) {
    asm("" : "+v"(v));
    return (f16)v;
}

// reflection without repeating the edge, folded as often as needed (period 2 (n - 1)); 0 for n == 1
__device__ __forceinline__ int seg_refl(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// the horizontal pass of 8 channels of token (row, x): acc = fmaf(w[dx], q, acc) from 0 over dx = -R .. R ascending
__device__ __forceinline__ void seg_hpass(const f16* qrow, int ldq, int x, int gw, const float* taps, int R, float (&acc)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
    for (int d = -R; d <= R; ++d) {
        U4H8 u;
        u.u = *reinterpret_cast<const uint4*>(qrow + (int64_t)seg_refl(x + d, gw) * ldq);
        const float w = taps[d + R];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, (float)u.e[j], acc[j]);
    }
}

// grid = (chunk groups, bands, blurred samples); cc chunks of 8 channels per block; band rows [y0, y0 + th)
__global__ __launch_bounds__(SEG_THREADS) void seg_blur_lds_kernel(const f16* q, f16* qb, int gh, int gw, int HD, int ldq, int64_t sq,
                                                                 const float* taps, int R, int th, int cc, int rows_cap) {
    extern __shared__ float hp[];       // [hull rows][gw][cc][8]
    const int b = blockIdx.z;
    const int y0 = blockIdx.y * th, y1 = min(y0 + th, gh);
    const int c0 = blockIdx.x * cc * 8;
    const int ncc = min(cc, HD / 8 - blockIdx.x * cc);
    // the hull of refl(y + dy, gh) over the band: [r_lo, r_hi]
    const int lo = y0 - R, hi = y1 - 1 + R;
    int r_lo = max(lo, 0), r_hi = min(hi, gh - 1);
    if (lo < 0) r_hi = max(r_hi, min(-lo, gh - 1));
    if (hi > gh - 1) r_lo = min(r_lo, max(2 * (gh - 1) - hi, 0));
    const int rows = min(r_hi - r_lo + 1, rows_cap);     // (the host sized rows_cap to hold the hull)
    const f16* qs = q + (int64_t)b * sq + c0;
    const int per_row = gw * ncc;
    for (int i = threadIdx.x; i < rows * per_row; i += SEG_THREADS) {
        const int r = i / per_row, rem = i - r * per_row;
        const int x = rem / ncc, c = rem - x * ncc;
        float acc[8];
        seg_hpass(qs + (int64_t)(r_lo + r) * gw * ldq + c * 8, ldq, x, gw, taps, R, acc);
        float* dst = hp + ((size_t)(r * gw + x) * cc + c) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j] = acc[j];
    }
    __syncthreads();
    f16* os = qb + ((int64_t)b * gh * gw) * HD + c0;
    for (int i = threadIdx.x; i < (y1 - y0) * per_row; i += SEG_THREADS) {
        const int yy = i / per_row, rem = i - yy * per_row;
        const int x = rem / ncc, c = rem - x * ncc;
        const int y = y0 + yy;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
        for (int d = -R; d <= R; ++d) {
            const int r = min(max(seg_refl(y + d, gh) - r_lo, 0), rows - 1);
            const float* src = hp + ((size_t)(r * gw + x) * cc + c) * 8;
            const float w = taps[d + R];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, src[j], acc[j]);
        }
        U4H8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.e[j] = seg_round_f16(acc[j]);
        *reinterpret_cast<uint4*>(os + ((int64_t)y * gw + x) * HD + c * 8) = o.u;
    }
}

// the same arithmetic without LDS: one work item = 8 channels of one token, the horizontal chain recomputed per vertical tap
__global__ __launch_bounds__(SEG_THREADS) void seg_blur_direct_kernel(const f16* q, f16* qb, int gh, int gw, int HD, int ldq, int64_t sq,
                                                                    const float* taps, int R, size_t work) {
    const int chunks = HD / 8;
    const size_t per_sample = (size_t)gh * gw * chunks;
    const size_t stride = (size_t)gridDim.x * SEG_THREADS;
    for (size_t t = (size_t)blockIdx.x * SEG_THREADS + threadIdx.x; t < work; t += stride) {
        const size_t b = t / per_sample, r0 = t - b * per_sample;
        const int n = (int)(r0 / chunks), c = (int)(r0 - (size_t)n * chunks);
        const int y = n / gw, x = n - y * gw;
        const f16* qs = q + (int64_t)b * sq + c * 8;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
        for (int d = -R; d <= R; ++d) {
            float h[8];
            seg_hpass(qs + (int64_t)seg_refl(y + d, gh) * gw * ldq, ldq, x, gw, taps, R, h);
            const float w = taps[d + R];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(w, h[j], acc[j]);
        }
        U4H8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.e[j] = seg_round_f16(acc[j]);
        *reinterpret_cast<uint4*>(qb + ((int64_t)b * gh * gw + n) * HD + c * 8) = o.u;
    }
}

// grid = (chunks, blurred samples): the mean query of 8 channels of one sample, broadcast to its N rows
__global__ __launch_bounds__(SEG_THREADS) void seg_mean_kernel(const f16* q, f16* qb, int N, int HD, int ldq, int64_t sq) {
    __shared__ float part[SEG_THREADS][8];
    const int b = blockIdx.y, c = blockIdx.x;
    const f16* qs = q + (int64_t)b * sq + c * 8;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
    for (int n = threadIdx.x; n < N; n += SEG_THREADS) {
        U4H8 u;
        u.u = *reinterpret_cast<const uint4*>(qs + (int64_t)n * ldq);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (float)u.e[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[threadIdx.x][j] = acc[j];
    __syncthreads();
    for (int s = SEG_THREADS / 2; s > 0; s >>= 1) {     // a fixed tree: thread t adds the partial of t + s
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) part[threadIdx.x][j] += part[threadIdx.x + s][j];
        }
        __syncthreads();
    }
    const float fn = (float)N;
    U4H8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.e[j] = seg_round_f16(part[0][j] / fn);
    f16* os = qb + ((int64_t)b * N) * HD + c * 8;
    for (int n = threadIdx.x; n < N; n += SEG_THREADS) *reinterpret_cast<uint4*>(os + (int64_t)n * HD) = o.u;
}

}  // namespace

extern "C" int vd_attention_qblur_f16(const void* q, const void* k, const void* v, void* out, int B, int H, int Nq, int Nk, int D,
                                      int ldq, int ldk, int ldv, int ldo, int64_t sq, int64_t sk, int64_t sv, int64_t so,
                                      float scale, int causal, int blur_from, int gh, int gw, const float* taps, int R, void* qb,
                                      hipStream_t stream) {
    VD_REQUIRE(q && k && v && out, "vd_attention_qblur_f16: null pointer");
    VD_REQUIRE(B > 0 && H > 0 && Nq > 0 && Nk > 0 && D > 0, "vd_attention_qblur_f16: empty problem B=%d H=%d Nq=%d Nk=%d D=%d", B, H,
               Nq, Nk, D);
    VD_REQUIRE(Nq == Nk, "vd_attention_qblur_f16: the query blur needs self-attention, Nq = %d and Nk = %d differ", Nq, Nk);
    VD_REQUIRE(causal == 0, "vd_attention_qblur_f16: no causal mask (causal = %d)", causal);
    VD_REQUIRE(blur_from >= 0 && blur_from <= B, "vd_attention_qblur_f16: blur_from = %d is outside [0, %d]", blur_from, B);
    VD_REQUIRE(gh > 0 && gw > 0 && (int64_t)gh * gw == Nq, "vd_attention_qblur_f16: the token grid %d x %d does not hold Nq = %d tokens",
               gh, gw, Nq);
    VD_REQUIRE(R >= -1, "vd_attention_qblur_f16: R = %d, expected a tap radius >= 0 or -1 (the mean query)", R);
    VD_REQUIRE(R < 0 || taps, "vd_attention_qblur_f16: R = %d needs the 2 R + 1 taps", R);
    VD_REQUIRE(R < 0 || ((uintptr_t)taps & 3) == 0, "vd_attention_qblur_f16: taps must be 4-byte aligned");
    const int64_t HD = (int64_t)H * D;
    VD_REQUIRE(HD % 8 == 0 && ldq % 8 == 0 && sq % 8 == 0,
               "vd_attention_qblur_f16: H * D = %lld, ldq = %d and the sample stride of q must be multiples of 8", (long long)HD, ldq);
    VD_REQUIRE(ldq >= HD, "vd_attention_qblur_f16: ldq = %d must cover the H * D = %lld columns", ldq, (long long)HD);
    VD_REQUIRE(vd_aligned16(q), "vd_attention_qblur_f16: q must be 16-byte aligned (a column offset that is a multiple of 8)");
    VD_REQUIRE(blur_from == B || (qb && vd_aligned16(qb)), "vd_attention_qblur_f16: the workspace qb must be a 16-byte aligned pointer");
    int rc = VD_OK;
    if (blur_from > 0)
        rc = vd_attention_f16(q, k, v, out, blur_from, H, Nq, Nk, D, ldq, ldk, ldv, ldo, sq, sk, sv, so, scale, 0, stream);
    if (rc >= 0 && blur_from < B) {
        const int Bp = B - blur_from;
        const f16* q0 = (const f16*)q + (int64_t)blur_from * sq;
        const int chunks = (int)(HD / 8);
        if (R < 0) {
            hipLaunchKernelGGL(seg_mean_kernel, dim3(chunks, Bp), dim3(SEG_THREADS), 0, stream, q0, (f16*)qb, Nq, (int)HD, ldq, sq);
        } else {
            // band height and channel chunks per block: the band's hull, at most min(gh, th + 2 R) rows, has to fit in LDS
            const int cc = chunks % 4 == 0 ? 4 : (chunks % 2 == 0 ? 2 : 1);
            int use_cc = 0, th = 0, rows = 0;
            for (int c = cc; c >= 1 && !use_cc; c >>= 1) {
                const int64_t cap = SEG_LDS_BYTES / ((int64_t)gw * c * 32);
                for (int t = min(SEG_BAND, gh); t >= 1; --t) {
                    const int64_t need = min((int64_t)gh, (int64_t)t + 2 * (int64_t)R);
                    if (need <= cap) {
                        use_cc = c, th = t, rows = (int)need;
                        break;
                    }
                }
            }
            if (use_cc && (gh + th - 1) / th <= 65535 && Bp <= 65535) {
                const size_t lds = (size_t)rows * gw * use_cc * 32;
                hipLaunchKernelGGL(seg_blur_lds_kernel, dim3((chunks + use_cc - 1) / use_cc, (gh + th - 1) / th, Bp), dim3(SEG_THREADS), lds,
                                   stream, q0, (f16*)qb, gh, gw, (int)HD, ldq, sq, taps, R, th, use_cc, rows);
            } else {
                const size_t work = (size_t)Bp * Nq * chunks;
                hipLaunchKernelGGL(seg_blur_direct_kernel, dim3(grid_for(work, SEG_THREADS, 4096)), dim3(SEG_THREADS), 0, stream, q0,
                                   (f16*)qb, gh, gw, (int)HD, ldq, sq, taps, R, work);
            }
        }
        rc = vd_check_launch("vd_attention_qblur_f16");
        if (rc < 0) return rc;
        rc = vd_attention_f16(qb, (const f16*)k + (int64_t)blur_from * sk, (const f16*)v + (int64_t)blur_from * sv,
                              (f16*)out + (int64_t)blur_from * so, Bp, H, Nq, Nk, D, (int)HD, ldk, ldv, ldo, (int64_t)Nq * HD, sk, sv, so,
                              scale, 0, stream);
    }
    if (rc < 0) {
        char inner[400];
        snprintf(inner, sizeof(inner), "%s", vd_last_error());
        vd_set_error("vd_attention_qblur_f16: %s", inner);
    }
    return rc;
}
