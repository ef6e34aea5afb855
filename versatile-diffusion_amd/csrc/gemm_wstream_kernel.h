// Weight-streaming GEMM for the long-K, small-M projections of the UNet's deep levels (round 4): y = x W^T with M = 2048 / 512
// rows against N x K = 1280 x 5120 -- the output projection of the gated feed-forward at the 16x16 / 8x8 levels
// (/root/reference/lib/model_zoo/attention.py:37-64: FeedForward.net[2]).  Included by conv_wstream.hip (vd_gemm_wstream_f16).
//
// gemm_f16_kernel brings BOTH operands of a 128 x 128 tile through LDS by LDS-DMA and spends 0.77 us per 64-deep k-step with
// 0.43 us of MFMAs in it (tools/probes/gemm_timeline.py).  The weights of a layer are static: here they are packed once in
// MFMA-fragment order (vd_hip/pack.py: pack_linear_weight_stream, [N / 32][K / 64][4 k-steps][64 lanes][8 halfs]) and go
// global -> registers as fully coalesced 1-KiB loads, two chunks (8 k-steps) ahead; only the activation tile
// ([128 rows][64 k] = 16 KiB per chunk, double-buffered, one barrier per chunk) takes the LDS path.  conv3x3_wstream_kernel
// without the taps: a block = 4 waves x 64 output columns over the same 128 rows, 8 MFMAs per k-step and wave from 2 weight
// fragments (registers) + 4 row fragments (LDS).  K is split over 64-deep chunks across blocks; the fp32 slabs go to the split-K
// reduce kernels of gemm.hip, which run the fused epilogue (bias, residual, statistics).
#pragma once
#include "gemm_kernel.h"

namespace {

struct GwArgs {
    const f16* a; const uint4* wp; float* ws;
    int lda, M, N;
    int nchunks, cps;          // 64-deep chunks of K: in total / per split
    int tiles_m, tiles_n, nsplit;
    unsigned a_bytes;
};
// ... with the second activation source of the concatenated entry (vd_gemm_wstream_cat_f16): chunks c >= c0_chunks of the K axis
// come from a1.  (A struct of its own: the kernel arguments of the single-source instance stay what they were.)
struct GwCatArgs : GwArgs {
    const f16* a1;
    int lda1, c0_chunks;
    unsigned a1_bytes;
};

// ... of the whole-K entry with the fused epilogue (vd_gemm_wstream_epi_f16): nsplit == 1, no slabs (ws unused); the epilogue of
// gemm_f16_kernel (LayerNorm fold, bias, GEGLU, alpha) runs on the accumulators where they sit.  N may end inside a block's 256
// columns (N % 64 == 0): a wave whose 64 columns lie past N streams the last valid panel instead -- every wave issues the same
// requests, the hand-counted waits of the chunk sequence hold in all of them -- and skips MFMAs and epilogue.
struct GwEpiArgs : GwArgs {
    f16* out;
    const f16* bias;         // [N] (packed order with GEGLU), read when flags has VD_EPI_BIAS
    const float* colsum;     // VD_EPI_LNFOLD: [N]
    const float* ln_stats;   // VD_EPI_LNFOLD: (mean, rstd) per row, or the int64 row sums with VD_EPI_LN_SUMS
    int ldc, flags, act, K;
    float alpha, ln_eps;
};

constexpr int GW_TILE = 128 * 128;   // bytes of one activation tile [128 rows][64 halfs]
constexpr int GW_MAXC = 32;          // chunks per block (the chunk sequence is unrolled)
constexpr int GW_MAXC_LONG = 34;     // ... of the long instance: K = 6400 (A = [h | x2], 5 x 1280) as 3 splits -- 240 blocks, one round

template <int LO, int HI, class F>
__device__ __forceinline__ void gw_static_for(F&& f) {
    if constexpr (LO < HI) {
        f(std::integral_constant<int, LO>{});
        gw_static_for<LO + 1, HI>(f);
    }
}

// MAXC: length of the unrolled chunk sequence.  P = GwCatArgs: the K axis is the concatenation of two activation matrices; the
// weights stay ONE fragment-order stream over the concatenated K.
// ---- fused epilogue of the whole-K instance (P = GwEpiArgs).  A lane owns row i * 32 + l31 and the columns j * 32 + 8 g + 4 hi ..
// + 3 of its wave's 64 -- the ownership of gemm_f16_kernel's accumulators -- and the float sequence is that kernel's (part 1 of its
// epilogue in gemm_kernel.h), operation for operation: fold  fmaf(rstd, acc, nmr * colsum[n]) + bias'[n]  for GEGLU,
// fmaf(rstd, acc, fmaf(nmr, colsum[n], bias'[n])) * alpha  plain, with rstd = 1 and no colsum term without the fold.  With the
// GEGLU packing ([32 value | 32 gate] per 64 weight rows) a wave's j = 0 tile holds the values and j = 1 the gates of its 32 outputs.
// Wait counts: the operands (row statistics, colsum, bias) are requested BEHIND the last chunk, as compiler-tracked loads -- they
// enter no hand-counted wait of the chunk sequence; the clamped weight re-reads still in flight are older and retire first.
// The fp16 tile leaves through the two activation buffers, free after the last chunk once every wave has passed the barrier in
// front (another wave may still read the last tile): a wave owns 8 KiB -- [128 rows][32 outputs] with GEGLU, else [64 rows][64
// columns] in two passes -- swizzled as the operand tiles are, and stores it as 16-byte segments of 64- / 128-byte row runs.
__device__ __forceinline__ void gw_epilogue(const GwEpiArgs& p, const f32x16 (&acc)[4][2], char* smem, int m0, int n0, bool active,
                                            int wave_s, int lane) {
    const int hi = lane >> 5, l31 = lane & 31;
    const bool lnf = (p.flags & VD_EPI_LNFOLD) != 0, ln_sums = (p.flags & VD_EPI_LN_SUMS) != 0;
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    uint4 lnst_r[4];
    U2H4 bias_r[8];
    float4 cs_r[8];
    {
        EpiCtx e = {};
        e.bias = p.bias;
        e.flags = p.flags;
        epi_load_bias<2>(e, p.N, n0 + 4 * hi, bias_r, true);   // columns past N (a wave that is not active) read zeros
        epi_load_lnstats<4>(p.ln_stats, p.M, 0, m0 + l31, lnst_r, lnf, ln_sums, p.M);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.colsum), 0, lnf ? p.N * 4 : 0, 0x00020000);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const vd_u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, (n0 + j * 32 + 8 * g + 4 * hi) * 4, 0, 0);
                cs_r[j * 4 + g] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
            }
    }
    __syncthreads();   // every wave has left the last activation tile
    char* cs = smem + wave_s * 8192;
    auto row_stats = [&](int i, float& ln_rstd, float& ln_nmr) {   // y = rstd * acc - (mean * rstd) * colsum[n] + bias'[n]
        ln_rstd = 1.f;
        ln_nmr = 0.f;
        if (lnf) {
            const uint4 st = lnst_r[i];
            if (ln_sums) {   // (sum, sum of squares) from the producer's row_sums
                ln_sums_decode(st, p.K, p.ln_eps, ln_rstd, ln_nmr);
            } else {
                ln_rstd = __uint_as_float(st.y);
                ln_nmr = -__uint_as_float(st.x) * ln_rstd;
            }
        }
    };
    if (p.act == VD_ACT_GEGLU) {
        if (active) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float ln_rstd, ln_nmr;
                row_stats(i, ln_rstd, ln_nmr);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const U2H4 bv = bias_r[g], bg = bias_r[4 + g];
                    float4 cv = make_float4(0.f, 0.f, 0.f, 0.f), cg = cv;
                    if (lnf) {
                        cv = cs_r[g];
                        cg = cs_r[4 + g];
                    }
                    const float cva[4] = {cv.x, cv.y, cv.z, cv.w}, cga[4] = {cg.x, cg.y, cg.z, cg.w};
                    U2H4 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float v = fmaf(ln_rstd, acc[i][0][g * 4 + q], ln_nmr * cva[q]) + (float)bv.e[q];
                        const float gt = fmaf(ln_rstd, acc[i][1][g * 4 + q], ln_nmr * cga[q]) + (float)bg.e[q];
                        o.e[q] = (f16)(v * vd_gelu_erf(gt) * p.alpha);
                    }
                    *reinterpret_cast<uint2*>(cs + lds_off_kb<32>(i * 32 + l31, g) + hi * 8) = o.u;
                }
            }
        }
        __syncthreads();
        if (active) {
            f16* dst = p.out + (size_t)m0 * p.ldc + (n0 >> 1);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int s = k * 64 + lane, row = s >> 2, slot = s & 3;
                *reinterpret_cast<uint4*>(dst + (size_t)row * p.ldc + slot * 8) = *reinterpret_cast<const uint4*>(cs + lds_off_kb<32>(row, slot));
            }
        }
    } else {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            if (pass > 0) __syncthreads();   // the stores of the previous pass have read the tile
            if (active) {
#pragma unroll
                for (int ii = 0; ii < 2; ++ii) {
                    const int i = pass * 2 + ii;
                    float ln_rstd, ln_nmr;
                    row_stats(i, ln_rstd, ln_nmr);
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            float bq[4] = {0.f, 0.f, 0.f, 0.f};
                            if (p.flags & VD_EPI_BIAS) {
                                const U2H4 t = bias_r[j * 4 + g];
#pragma unroll
                                for (int q = 0; q < 4; ++q) bq[q] = (float)t.e[q];
                            }
                            if (lnf) {
                                const float4 c4 = cs_r[j * 4 + g];
                                bq[0] = fmaf(ln_nmr, c4.x, bq[0]);
                                bq[1] = fmaf(ln_nmr, c4.y, bq[1]);
                                bq[2] = fmaf(ln_nmr, c4.z, bq[2]);
                                bq[3] = fmaf(ln_nmr, c4.w, bq[3]);
                            }
                            U2H4 o;
#pragma unroll
                            for (int q = 0; q < 4; ++q) o.e[q] = (f16)(fmaf(ln_rstd, acc[i][j][g * 4 + q], bq[q]) * p.alpha);
                            *reinterpret_cast<uint2*>(cs + lds_off_kb<64>(ii * 32 + l31, j * 4 + g) + hi * 8) = o.u;
                        }
                }
            }
            __syncthreads();
            if (active) {
                f16* dst = p.out + (size_t)(m0 + pass * 64) * p.ldc + n0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int s = k * 64 + lane, row = s >> 3, slot = s & 7;
                    *reinterpret_cast<uint4*>(dst + (size_t)row * p.ldc + slot * 8) = *reinterpret_cast<const uint4*>(cs + lds_off_kb<64>(row, slot));
                }
            }
        }
    }
}

// P = GwEpiArgs: the whole K in one block, the fused epilogue in place of the slab store, two blocks per CU (one wave of each per
// SIMD: a block keeps the matrix pipe about 40 % busy).
template <int MAXC, class P>
__global__ __launch_bounds__(256, (std::is_same<P, GwEpiArgs>::value ? 2 : 1)) void gemm_wstream_kernel(const P p) {
    constexpr bool CAT = std::is_same<P, GwCatArgs>::value;
    constexpr bool EPI = std::is_same<P, GwEpiArgs>::value;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const int hi = lane >> 5, l31 = lane & 31;

    // blocks that share a weight panel (same column slice and K split, the tiles_m row tiles) get consecutive logical indices
    // inside one XCD's contiguous run: the panel comes from HBM once and hits that L2 for the other row tiles
    const int ntot = gridDim.x;
    int bid = blockIdx.x;
    {
        const int q = ntot >> 3, r = ntot & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tm = bid % p.tiles_m;
    const int rest = bid / p.tiles_m;
    const int tn = rest % p.tiles_n;
    const int split = rest / p.tiles_n;
    const int m0 = tm * 128;
    const int n0 = tn * 256 + wave_s * 64;
    const int c_begin = split * p.cps;
    int c_end = c_begin + p.cps;
    if (c_end > p.nchunks) c_end = p.nchunks;
    const int ncl = c_end - c_begin;   // >= 1 by construction of the launcher

    const i32x4 rs_a = make_rsrc_words(p.a, p.a_bytes);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

    // ---- activation tile of a chunk: 16 pieces of 8 rows x 128 bytes, wave w issues pieces w, w + 4, w + 8, w + 12.  The DMA
    // destination is lane-linear (row = 8 q + lane / 8, physical slot = lane % 8), so the XOR swizzle of the LDS image
    // (lds_off_kb<64>) is applied on the source side: the lane fetches the logical slot that lives at its physical slot
    unsigned avoff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = (j * 4 + wave) * 8 + (lane >> 3);
        const int row = m0 + r;
        avoff[j] = row < p.M ? (unsigned)((row * p.lda + (((lane & 7) ^ lds_swz<64>(r)) << 3)) * 2) : OOB_OFFSET;
    }
    // second source: its own descriptor and row offsets (another leading dimension); which of the two a chunk reads is decided
    // per chunk on wave-uniform values -- descriptor and column offset in scalar registers
    i32x4 rs_a1 = rs_a;
    unsigned avoff1[4];
    if constexpr (CAT) {
        rs_a1 = make_rsrc_words(p.a1, p.a1_bytes);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = (j * 4 + wave) * 8 + (lane >> 3);
            const int row = m0 + r;
            avoff1[j] = row < p.M ? (unsigned)((row * p.lda1 + (((lane & 7) ^ lds_swz<64>(r)) << 3)) * 2) : OOB_OFFSET;
        }
    }
    auto issue_a = [&](int c, int buf) {
        if constexpr (CAT) {
            const bool second = c >= p.c0_chunks;
            const i32x4 rs = second ? rs_a1 : rs_a;
            const unsigned soff = (unsigned)((second ? c - p.c0_chunks : c) * 128);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                dma16(rs, lds0 + (unsigned)(buf * GW_TILE + (j * 4 + wave_s) * 1024), second ? avoff1[j] : avoff[j], soff);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                dma16(rs_a, lds0 + (unsigned)(buf * GW_TILE + (j * 4 + wave_s) * 1024), avoff[j], (unsigned)(c * 128));
        }
    };

    // ---- weight stream of this wave: two n tiles, 4 fragments (1 KiB each) per chunk and tile, chunks contiguous
    bool active = true;   // EPI: false in a wave whose columns lie past N (wave-uniform)
    int nt0 = n0 >> 5;
    if constexpr (EPI) {
        active = n0 < p.N;
        if (!active) nt0 = (p.N >> 5) - 2;
    }
    const uint4* wq0 = p.wp + (size_t)nt0 * p.nchunks * 256 + lane;
    const uint4* wq1 = p.wp + (size_t)(nt0 + 1) * p.nchunks * 256 + lane;
    const int c_last = c_end - 1;
    U4H8 wf[2][4][2];   // [chunk parity][k-step][n tile]
    auto load_w = [&](auto pt, auto st, int c) {   // fragments of k-step s of chunk c (clamped: the tail re-reads the last chunk)
        constexpr int par = decltype(pt)::value, s = decltype(st)::value;
        const int cc = c < c_last ? c : c_last;
        wf[par][s][0].u = wq0[((size_t)cc * 4 + s) * 64];
        wf[par][s][1].u = wq1[((size_t)cc * 4 + s) * 64];
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // row fragments: lane row m = i * 32 + l31 of the block's 128, logical slot 2 ks + hi (the swizzle key of row i * 32 + l31
    // is that of l31)
    int rd[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) rd[ks] = lds_off_kb<64>(l31, ks * 2 + hi);

    // ---- prologue: activation tile of the first chunk, weights of the first two chunks
    issue_a(c_begin, 0);
    gw_static_for<0, 4>([&](auto st) { load_w(std::integral_constant<int, 0>{}, st, c_begin); });
    gw_static_for<0, 4>([&](auto st) { load_w(std::integral_constant<int, 1>{}, st, c_begin + 1); });

    auto chunk = [&](auto lt) {
        constexpr int lc = decltype(lt)::value, par = lc & 1;
        const std::integral_constant<int, par> pt;
        const int c = c_begin + lc;
        // this chunk's activation tile (requested during the previous chunk, in front of the 8 weight loads of chunk c + 1) and
        // its weights (requested two chunks ago) have landed for this wave ... for every wave; every wave has left chunk c - 1,
        // whose buffer the DMA below refills.  Requests in flight here, oldest first: W(lc) [8, from chunk lc - 2 or the
        // prologue], A(lc) [4] and W(lc + 1) [8] (both from chunk lc - 1, the tile first): a count of 8 retires all but W(lc + 1).
        // Chunk MAXC - 2 is the first that requests no weights (chunk MAXC does not exist, see below), so at chunk MAXC - 1 --
        // and only there, whatever MAXC is -- the tile is the newest request in flight: a count of 8 would not cover it
        wait_vm<(lc + 1 < MAXC ? 8 : 0)>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (lc + 1 < ncl) issue_a(c + 1, par ^ 1);
        const char* st = smem + par * GW_TILE;
        gw_static_for<0, 4>([&](auto kt) {
            constexpr int ks = decltype(kt)::value;
            if (!EPI || active) {
                f16x8 bf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    U4H8 v;
                    v.u = *reinterpret_cast<const uint4*>(st + rd[ks] + i * 32 * 128);
                    bf[i] = v.h;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[par][ks][j].h, bf[i], acc[i][j], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // issued whether or not chunk c + 2 is this block's (clamped): every chunk adds exactly 8 weight loads behind its
            // DMA pieces -- except where no block has a chunk lc + 2, which the wait of chunk lc + 1 above accounts for
            if constexpr (lc + 2 < MAXC) load_w(pt, kt, c + 2);
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    // No loop: the chunks of a block (at most MAXC, the launcher splits K accordingly) are unrolled behind forward guards.
    // With a back edge hipcc cannot count the weight loads that are in flight ACROSS iterations and puts s_waitcnt vmcnt(0) in
    // front of the first MFMA of every iteration -- the ring drained once per trip (conv3x3_wstream_kernel pays that once per
    // 36-k-step chunk; here it would be every second 4-k-step chunk).
    gw_static_for<0, MAXC>([&](auto lt) {
        constexpr int lc = decltype(lt)::value;
        if (lc < ncl) chunk(lt);
    });

    if constexpr (EPI) {
        gw_epilogue(p, acc, smem, m0, n0, active, wave_s, lane);
    } else {
        // ---- fp32 slab of this split for the reduce kernel, straight from registers (4 consecutive floats per lane and group)
        float* base = p.ws + (size_t)split * (size_t)p.M * p.N;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + i * 32 + l31;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = n0 + j * 32 + 8 * g + 4 * hi;
                    if (row < p.M)
                        *reinterpret_cast<float4*>(base + (size_t)row * p.N + col) =
                            make_float4(acc[i][j][g * 4], acc[i][j][g * 4 + 1], acc[i][j][g * 4 + 2], acc[i][j][g * 4 + 3]);
                }
        }
    }
}

}  // namespace
