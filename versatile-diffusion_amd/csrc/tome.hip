// Token merging for self-attention (Bolya & Hoffman, "Token Merging for Fast Stable Diffusion", 2023; the tomesd package with
// sx = sy = 2, use_rand = False) on gfx950: the four launches a merging block adds.  Contracts (sets, tie rules, roundings):
// include/vd_hip.h.
//
// vd_tome_match_f16: per sample the [Ns x C] x [C x Nd] cosine-similarity product with a running (max, argmax) per source row;
//   the score matrix never reaches memory.  Block = 4 waves, wave w owns 32 sources whose rows sit in registers as the B operand of
//   v_mfma_f32_32x32x16_f16 for the whole kernel; destination rows go through LDS in tiles of 32 as the A operand, so S^T
//   (destinations x sources) has ONE source per lane (column lane & 31) and 16 destinations in its registers, ascending with the
//   register index: the running argmax is lane-local, a strict > keeps the lowest d, and the two lane halves are combined once at the
//   end (attention.hip's swapped product).  The next tile is fetched into registers while the current one is multiplied; the row
//   norms come from the same registers (8 lanes per row, a fixed shuffle tree: the same bits every run).
// vd_tome_plan: rank by counting (Ns^2 compares per sample against values staged in LDS) -> row_of.
// vd_tome_merge_f16: a block owns 8 destinations, lists the sources merged into them in LDS (one scan of row_of) and sums in
//   registers as int64 multiples of 2^-24 -- exact, so the order of the list does not matter; no atomics on the data tensor.
// vd_tome_unmerge_f16: a 16-byte row gather.
#include <stdio.h>

#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

constexpr int TM_THREADS = 256;
constexpr int TM_DT = 32;            // destinations per LDS tile
constexpr int TM_SRC_PER_BLOCK = 128; // 4 waves x 32 sources
constexpr int TM_DPB = 8;            // destinations per merge block
constexpr int TM_MAX_NS = 12288;     // sources per sample the merge lists in LDS (48 KiB): grids up to 128 x 128

// source ordinal -> token, destination ordinal -> token (grid H x W, both even; W2 = W / 2)
__device__ __forceinline__ int tm_src_token(int i, int W, int W2) {
    const int per = W + W2;                 // sources of a row pair: W / 2 in the even row, W in the odd one
    const int p = i / per, rem = i - p * per;
    return rem < W2 ? (2 * p) * W + 2 * rem + 1 : (2 * p + 1) * W + (rem - W2);
}
__device__ __forceinline__ int tm_dst_token(int d, int W, int W2) {
    const int q = d / W2;
    return (2 * q) * W + 2 * (d - q * W2);
}
// token -> ordinal in its set; *is_dst tells which
__device__ __forceinline__ int tm_ordinal(int n, int W, int W2, bool* is_dst) {
    const int y = n / W, x = n - y * W;
    if (!(y & 1) && !(x & 1)) {
        *is_dst = true;
        return (y >> 1) * W2 + (x >> 1);
    }
    *is_dst = false;
    const int base = (y >> 1) * (W + W2);
    return (y & 1) ? base + W2 + x : base + (x >> 1);
}

__device__ __forceinline__ float tm_sumsq(const U4H8& v) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s = fmaf((float)v.e[j], (float)v.e[j], s);
    return s;
}
__device__ __forceinline__ float tm_inv(float s) { return s > 0.f ? 1.0f / sqrtf(s) : 0.f; }

// KS = C / 16 MFMA k-steps.  LDS: [TM_DT][C + 8] fp16 (row pitch an odd number of 16-byte chunks: the ds_read_b128 of 32 rows is
// conflict-free) + TM_DT inverse norms.
template <int KS>
__global__ __launch_bounds__(TM_THREADS) void tome_match_kernel(const f16* __restrict__ h, int ldh, int64_t sample_stride, int H, int W,
                                                                int* __restrict__ node_idx, float* __restrict__ node_max) {
    constexpr int C = KS * 16;
    constexpr int PITCH = C + 8;
    constexpr int CH = C / 8;                      // 16-byte chunks per row
    constexpr int CPT = (CH + 7) / 8;              // chunks per thread when 8 threads share a row
    __shared__ __attribute__((aligned(16))) f16 tile[TM_DT * PITCH];
    __shared__ float dinv[TM_DT];

    const int W2 = W >> 1;
    const int N = H * W, Nd = N >> 2, Ns = N - Nd;
    const int b = blockIdx.y;
    const f16* hb = h + (int64_t)b * sample_stride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;

    // ---- this lane's source row as B-operand fragments: element j of k-step ks is column ks * 16 + hi * 8 + j
    const int i_src = blockIdx.x * TM_SRC_PER_BLOCK + wave * 32 + l31;
    const bool src_ok = i_src < Ns;
    f16x8 qf[KS];
    float ssq = 0.f;
    {
        const f16* row = hb + (int64_t)tm_src_token(src_ok ? i_src : 0, W, W2) * ldh;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            U4H8 v;      // (the load is unconditional, on a clamped row: a branch per load would serialise the fetches)
            v.u = *reinterpret_cast<const uint4*>(row + ks * 16 + hi * 8);
            if (!src_ok) v.u = make_uint4(0, 0, 0, 0);
            qf[ks] = v.h;
            ssq += tm_sumsq(v);
        }
    }
    const float inv_i = tm_inv(ssq + __shfl_xor(ssq, 32, 64));

    // ---- destination tiles: thread (row = tid / 8, sub = tid % 8) carries chunks sub, sub + 8, ... of its row
    const int trow = tid >> 3, sub = tid & 7;
    U4H8 pre[CPT];
    auto fetch = [&](const int t) __attribute__((always_inline)) {
        const int d = t * TM_DT + trow;
        const bool ok = d < Nd;
        const f16* row = hb + (int64_t)tm_dst_token(ok ? d : 0, W, W2) * ldh;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const int ch = sub + 8 * j;
            // unconditional loads on clamped addresses, all in flight together; what lies outside the tile is zeroed afterwards
            pre[j].u = *reinterpret_cast<const uint4*>(row + (ch < CH ? ch : CH - 1) * 8);
            if (!(ok && ch < CH)) pre[j].u = make_uint4(0, 0, 0, 0);
        }
    };
    auto put = [&]() __attribute__((always_inline)) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const int ch = sub + 8 * j;
            if (ch < CH) *reinterpret_cast<uint4*>(tile + trow * PITCH + ch * 8) = pre[j].u;
            s += tm_sumsq(pre[j]);
        }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (sub == 0) dinv[trow] = tm_inv(s);
    };

    float best = -INFINITY;
    int best_d = 0;
    const int ntiles = (Nd + TM_DT - 1) / TM_DT;
    fetch(0);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();          // every wave has left tile t - 1
        put();
        __syncthreads();          // tile t is in LDS
        if (t + 1 < ntiles) fetch(t + 1);   // in flight while this tile is multiplied
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        // A fragments in groups of G, the next group's reads issued in front of this group's MFMAs (one register set per parity):
        // the LDS latency is paid once per tile, not once per MFMA
        constexpr int G = (KS % 4 == 0) ? 4 : 2;
        constexpr int NG = KS / G;
        static_assert(KS % G == 0, "k-steps come in whole groups");
        const f16* arow = tile + l31 * PITCH + hi * 8;
        U4H8 af[2][G];
#pragma unroll
        for (int j = 0; j < G; ++j) af[0][j].u = *reinterpret_cast<const uint4*>(arow + j * 16);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) {
#pragma unroll
                for (int j = 0; j < G; ++j) af[(g + 1) & 1][j].u = *reinterpret_cast<const uint4*>(arow + ((g + 1) * G + j) * 16);
            }
            __builtin_amdgcn_sched_barrier(0);      // (left alone, the scheduler sinks every read to right in front of its MFMA)
#pragma unroll
            for (int j = 0; j < G; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[g & 1][j].h, qf[g * G + j], acc, 0, 0, 0);
        }
        // this lane's 16 destinations of the tile, ascending with r
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dl = (r & 3) + 8 * (r >> 2) + 4 * hi;
            const int d = t * TM_DT + dl;
            const float s = acc[r] * dinv[dl];
            if (d < Nd && s > best) {
                best = s;
                best_d = d;
            }
        }
    }
    // the other half's candidates: the greater score, at equal scores the lower d
    const float ob = __shfl_xor(best, 32, 64);
    const int od = __shfl_xor(best_d, 32, 64);
    if (ob > best || (ob == best && od < best_d)) {
        best = ob;
        best_d = od;
    }
    if (src_ok && hi == 0) {
        node_idx[(int64_t)b * Ns + i_src] = best_d;
        node_max[(int64_t)b * Ns + i_src] = best * inv_i;
    }
}

// rank[i] = #{j : v[j] > v[i] or (v[j] == v[i] and j < i)}; a block owns 64 sources (one per lane), its four waves count a quarter
// of every staged tile each and the partial ranks (integers: exact in any order) meet in LDS
constexpr int TP_TILE = 2048;
constexpr int TP_SRC = 64;
__global__ __launch_bounds__(TM_THREADS) void tome_plan_kernel(const int* __restrict__ node_idx, const float* __restrict__ node_max, int H,
                                                               int W, int r, int* __restrict__ row_of) {
    __shared__ __attribute__((aligned(16))) float vals[TP_TILE];
    __shared__ int part[TM_THREADS / TP_SRC][TP_SRC];
    const int W2 = W >> 1;
    const int N = H * W, Nd = N >> 2, Ns = N - Nd;
    const int b = blockIdx.y;
    const float* vm = node_max + (int64_t)b * Ns;
    const int lane = threadIdx.x & (TP_SRC - 1), q = threadIdx.x / TP_SRC;
    const int i = blockIdx.x * TP_SRC + lane;
    const bool ok = i < Ns;
    const float mine = ok ? vm[i] : 0.f;
    int rank = 0;
    for (int j0 = 0; j0 < Ns; j0 += TP_TILE) {
        const int cnt = min(TP_TILE, Ns - j0);
        __syncthreads();
        for (int j = threadIdx.x; j < TP_TILE; j += TM_THREADS) vals[j] = j < cnt ? vm[j0 + j] : __builtin_nanf("");
        __syncthreads();
        // j < i <=> j0 + jj < i: before the tile that holds i every equal value counts, behind it none
        const int lim = i - j0;     // entries jj < lim have j < i
        const int jb = q * (TP_TILE / (TM_THREADS / TP_SRC));
        const int je = min(jb + TP_TILE / (TM_THREADS / TP_SRC), cnt);
        for (int jj = jb; jj < je; jj += 4) {   // (the padding is NaN: neither greater than nor equal to anything)
            const float4 v = *reinterpret_cast<const float4*>(vals + jj);
            rank += (v.x > mine || (v.x == mine && jj + 0 < lim)) ? 1 : 0;
            rank += (v.y > mine || (v.y == mine && jj + 1 < lim)) ? 1 : 0;
            rank += (v.z > mine || (v.z == mine && jj + 2 < lim)) ? 1 : 0;
            rank += (v.w > mine || (v.w == mine && jj + 3 < lim)) ? 1 : 0;
        }
    }
    part[q][lane] = rank;
    __syncthreads();
    if (q != 0) return;
    rank = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
    static_assert(TM_THREADS / TP_SRC == 4, "four partial ranks");
    int* ro = row_of + (int64_t)b * N;
    if (ok) {
        const int n = tm_src_token(i, W, W2);
        ro[n] = rank >= r ? rank - r : (Ns - r) + node_idx[(int64_t)b * Ns + i];
    }
    if (i < Nd) ro[tm_dst_token(i, W, W2)] = (Ns - r) + i;
}

// fp16 bits -> the integer multiple of 2^-24 they stand for (finite values; |v| < 2^40)
__device__ __forceinline__ long long tm_fixed(unsigned short u) {
    const int e = (u >> 10) & 31, m = u & 1023;
    const long long mag = e ? (long long)(m | 1024) << (e - 1) : (long long)m;
    return (u & 0x8000) ? -mag : mag;
}
// double -> fp16 with ONE rounding to nearest even: to fp32 by round-to-odd (24 bits >= 11 + 2, so the second rounding sees
// everything the first one dropped), then the hardware's fp32 -> fp16 conversion
__device__ __forceinline__ f16 tm_round_f16(double q) {
    float f = (float)q;
    unsigned u = __float_as_uint(f);
    if (fabs((double)f) > fabs(q)) f = __uint_as_float(--u);   // rounded away from zero: back to the truncation
    if ((double)f != q) u |= 1u;                                 // inexact: odd
    float g = __uint_as_float(u);
    asm("" : "+v"(g));
    return (f16)g;
}

// blocks [0, dst_blocks): TM_DPB destinations each; the others copy the unmerged source rows (grid-stride)
__global__ __launch_bounds__(TM_THREADS) void tome_merge_kernel(const f16* __restrict__ x, int ldx, int64_t sx, int chunks,
                                                                const int* __restrict__ row_of, int H, int W, int r, f16* __restrict__ out,
                                                                int ldo, int64_t so, int dst_blocks) {
    extern __shared__ int members[];     // packed (token << 3 | local destination), at most Ns entries
    __shared__ int n_members;
    const int W2 = W >> 1;
    const int N = H * W, Nd = N >> 2, Ns = N - Nd;
    const int b = blockIdx.y;
    const int* ro = row_of + (int64_t)b * N;
    const f16* xb = x + (int64_t)b * sx;
    f16* ob = out + (int64_t)b * so;
    const int first_dst_row = Ns - r;
    if ((int)blockIdx.x >= dst_blocks) {
        const int nb = gridDim.x - dst_blocks;
        const size_t work = (size_t)N * chunks;
        for (size_t t = (size_t)(blockIdx.x - dst_blocks) * TM_THREADS + threadIdx.x; t < work; t += (size_t)nb * TM_THREADS) {
            const int n = (int)(t / chunks), c = (int)(t - (size_t)n * chunks);
            const int row = ro[n];
            if (row >= first_dst_row || row < 0) continue;       // a destination or a merged source (a row_of no plan wrote: skipped)
            *reinterpret_cast<uint4*>(ob + (int64_t)row * ldo + c * 8) = *reinterpret_cast<const uint4*>(xb + (int64_t)n * ldx + c * 8);
        }
        return;
    }
    const int d0 = blockIdx.x * TM_DPB;
    if (threadIdx.x == 0) n_members = 0;
    __syncthreads();
    if (r > 0) {
        for (int n = threadIdx.x; n < N; n += TM_THREADS) {
            bool is_dst;
            tm_ordinal(n, W, W2, &is_dst);
            if (is_dst) continue;
            const int ld = ro[n] - first_dst_row - d0;
            if (ld >= 0 && ld < TM_DPB) members[atomicAdd(&n_members, 1)] = (n << 3) | ld;
        }
    }
    __syncthreads();
    const int nm = n_members;
    for (int it = threadIdx.x; it < TM_DPB * chunks; it += TM_THREADS) {
        const int ld = it / chunks, c = it - ld * chunks;
        const int d = d0 + ld;
        if (d >= Nd) break;
        long long acc[8];
        U4H8 v;
        v.u = *reinterpret_cast<const uint4*>(xb + (int64_t)tm_dst_token(d, W, W2) * ldx + c * 8);
        int count = 1;
        if (nm == 0) {      // (also r == 0: the row is its own mean)
            *reinterpret_cast<uint4*>(ob + (int64_t)(first_dst_row + d) * ldo + c * 8) = v.u;
            continue;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = tm_fixed(__builtin_bit_cast(unsigned short, v.e[j]));
        for (int m = 0; m < nm; ++m) {
            const int e = members[m];
            if ((e & 7) != ld) continue;
            U4H8 s;
            s.u = *reinterpret_cast<const uint4*>(xb + (int64_t)(e >> 3) * ldx + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += tm_fixed(__builtin_bit_cast(unsigned short, s.e[j]));
            ++count;
        }
        if (count > 1) {
            const double dc = (double)count;
#pragma unroll
            for (int j = 0; j < 8; ++j) v.e[j] = tm_round_f16(ldexp((double)acc[j], -24) / dc);
        }
        *reinterpret_cast<uint4*>(ob + (int64_t)(first_dst_row + d) * ldo + c * 8) = v.u;
    }
}

__global__ __launch_bounds__(TM_THREADS) void tome_unmerge_kernel(const f16* __restrict__ a, int lda, int64_t sa, int chunks,
                                                                  const int* __restrict__ row_of, int N, int Nm, f16* __restrict__ out,
                                                                  int ldo, int64_t so, size_t work) {
    const size_t per_sample = (size_t)N * chunks;
    for (size_t t = (size_t)blockIdx.x * TM_THREADS + threadIdx.x; t < work; t += (size_t)gridDim.x * TM_THREADS) {
        const size_t b = t / per_sample, q = t - b * per_sample;
        const size_t n = q / chunks, c = q - n * chunks;
        const int row = min(max(row_of[b * N + n], 0), Nm - 1);     // (a valid plan is never clamped)
        *reinterpret_cast<uint4*>(out + (int64_t)b * so + (int64_t)n * ldo + c * 8) =
            *reinterpret_cast<const uint4*>(a + (int64_t)b * sa + (int64_t)row * lda + c * 8);
    }
}

// the checks every entry shares; what: the entry's name
int tm_grid_ok(const char* what, int B, int H, int W) {
    VD_REQUIRE(B > 0 && H > 0 && W > 0, "%s: empty problem B=%d H=%d W=%d", what, B, H, W);
    VD_REQUIRE(H % 2 == 0 && W % 2 == 0, "%s: the token grid %d x %d must be even on both sides", what, H, W);
    VD_REQUIRE((int64_t)H * W <= (1 << 24), "%s: the token grid %d x %d is too large", what, H, W);
    VD_REQUIRE(B <= 65535, "%s: B = %d exceeds the grid's 65535 samples", what, B);
    return VD_OK;
}

}  // namespace

extern "C" int vd_tome_match_f16(const void* h, int ldh, int64_t sample_stride, int B, int H, int W, int C, int* node_idx,
                                 float* node_max, hipStream_t stream) {
    VD_REQUIRE(h && node_idx && node_max, "vd_tome_match_f16: null pointer");
    if (int rc = tm_grid_ok("vd_tome_match_f16", B, H, W)) return rc;
    VD_REQUIRE(vd_aligned16(h) && ldh % 8 == 0 && sample_stride % 8 == 0 && ldh >= C,
               "vd_tome_match_f16: h must be 16-byte aligned with ldh = %d >= C and sample_stride multiples of 8", ldh);
    VD_REQUIRE(((uintptr_t)node_idx & 3) == 0 && ((uintptr_t)node_max & 3) == 0, "vd_tome_match_f16: misaligned node_idx / node_max");
    const int N = H * W, Ns = N - N / 4;
    const dim3 grid((Ns + TM_SRC_PER_BLOCK - 1) / TM_SRC_PER_BLOCK, B), block(TM_THREADS);
    const f16* hp = (const f16*)h;
    switch (C) {
#define TM_CASE(c)                                                                                                                 \
    case c:                                                                                                                        \
        hipLaunchKernelGGL(tome_match_kernel<c / 16>, grid, block, 0, stream, hp, ldh, sample_stride, H, W, node_idx, node_max); \
        break;
        TM_CASE(32)
        TM_CASE(64)
        TM_CASE(128)
        TM_CASE(320)
        TM_CASE(640)
#undef TM_CASE
        default:
            vd_set_error("vd_tome_match_f16: unsupported width C = %d (32, 64, 128, 320, 640)", C);
            return VD_ERR_UNSUPPORTED;
    }
    return vd_check_launch("vd_tome_match_f16");
}

extern "C" int vd_tome_plan(const int* node_idx, const float* node_max, int B, int H, int W, int r, int* row_of, hipStream_t stream) {
    VD_REQUIRE(node_idx && node_max && row_of, "vd_tome_plan: null pointer");
    if (int rc = tm_grid_ok("vd_tome_plan", B, H, W)) return rc;
    VD_REQUIRE((((uintptr_t)node_idx | (uintptr_t)node_max | (uintptr_t)row_of) & 3) == 0, "vd_tome_plan: misaligned pointer");
    const int N = H * W, Ns = N - N / 4;
    VD_REQUIRE(r >= 0 && r <= Ns, "vd_tome_plan: r = %d is outside [0, %d]", r, Ns);
    hipLaunchKernelGGL(tome_plan_kernel, dim3((Ns + TP_SRC - 1) / TP_SRC, B), dim3(TM_THREADS), 0, stream, node_idx, node_max, H, W,
                       r, row_of);
    return vd_check_launch("vd_tome_plan");
}

namespace {
int tm_rows_ok(const char* what, const void* in, int ldi, int64_t si, int cols, const int* row_of, int B, int H, int W, int r,
               const void* out, int ldo, int64_t so) {
    VD_REQUIRE(in && row_of && out, "%s: null pointer", what);
    if (int rc = tm_grid_ok(what, B, H, W)) return rc;
    VD_REQUIRE(cols > 0 && cols % 8 == 0, "%s: cols = %d must be a positive multiple of 8", what, cols);
    VD_REQUIRE(vd_aligned16(in) && vd_aligned16(out) && ldi % 8 == 0 && ldo % 8 == 0 && si % 8 == 0 && so % 8 == 0 && ldi >= cols &&
                   ldo >= cols,
               "%s: the tensors must be 16-byte aligned, their leading dimensions (%d, %d) >= cols and, like the sample strides, multiples of 8",
               what, ldi, ldo);
    VD_REQUIRE(((uintptr_t)row_of & 3) == 0, "%s: misaligned row_of", what);
    const int N = H * W, Ns = N - N / 4;
    VD_REQUIRE(r >= 0 && r <= Ns, "%s: r = %d is outside [0, %d]", what, r, Ns);
    return VD_OK;
}
}  // namespace

extern "C" int vd_tome_merge_f16(const void* x, int ldx, int64_t sx, int cols, const int* row_of, int B, int H, int W, int r,
                                 void* out, int ldo, int64_t so, hipStream_t stream) {
    if (int rc = tm_rows_ok("vd_tome_merge_f16", x, ldx, sx, cols, row_of, B, H, W, r, out, ldo, so)) return rc;
    const int N = H * W, Nd = N / 4, Ns = N - Nd;
    if (Ns > TM_MAX_NS) {
        vd_set_error("vd_tome_merge_f16: %d sources per sample exceed the %d the member list holds (grids up to 128 x 128)", Ns, TM_MAX_NS);
        return VD_ERR_UNSUPPORTED;
    }
    const int chunks = cols / 8;
    const int dst_blocks = (Nd + TM_DPB - 1) / TM_DPB;
    const int copy_blocks = r < Ns ? grid_for((size_t)N * chunks, TM_THREADS, 1024) : 0;
    hipLaunchKernelGGL(tome_merge_kernel, dim3(dst_blocks + copy_blocks, B), dim3(TM_THREADS), (size_t)Ns * sizeof(int), stream,
                       (const f16*)x, ldx, sx, chunks, row_of, H, W, r, (f16*)out, ldo, so, dst_blocks);
    return vd_check_launch("vd_tome_merge_f16");
}

extern "C" int vd_tome_unmerge_f16(const void* a, int lda, int64_t sa, int cols, const int* row_of, int B, int H, int W, int r,
                                   void* out, int ldo, int64_t so, hipStream_t stream) {
    if (int rc = tm_rows_ok("vd_tome_unmerge_f16", a, lda, sa, cols, row_of, B, H, W, r, out, ldo, so)) return rc;
    const int N = H * W, chunks = cols / 8;
    const size_t work = (size_t)B * N * chunks;
    hipLaunchKernelGGL(tome_unmerge_kernel, dim3(grid_for(work, TM_THREADS, 4096)), dim3(TM_THREADS), 0, stream, (const f16*)a, lda, sa,
                       chunks, row_of, N, N - r, (f16*)out, ldo, so, work);
    return vd_check_launch("vd_tome_unmerge_f16");
}
