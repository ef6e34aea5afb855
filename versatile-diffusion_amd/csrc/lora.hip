// LoRA adapters on gfx950: the merge of up to eight rank-r updates into one weight matrix.  Contract (operands, the written-out
// roundings): include/vd_hip.h.
//
// vd_lora_merge computes out[n][k] = base[n][k] + sum_a scale_a (up_a down_a)[n][k] with every fp32 operation spelled out: per
// element a chain of fmaf over the rank in ascending order, one fmaf per term in table order, one final rounding.  VALU fp32 on
// purpose: the order in which an MFMA sums its products is not ours to state, and the merge is bound by the one read and one write
// of the parameter anyway (a rank-16 term is about 32 flops per 8 bytes).
//   block   256 lanes own a 64 x 64 tile of out; lane (ty, tx) = (tid / 16, tid % 16) owns the 4 x 4 patch at rows 4 ty, columns
//           4 tx, so sixteen lanes of a wave cover 256 contiguous bytes of a row of an fp32 parameter
//   stage   per term the rank is walked in chunks of 32: up[64 x 32] goes to LDS transposed ([j][row], rows padded to 68 floats: a
//           16-byte-aligned row, the transposing 4-byte writes at most 4-way on a bank), down[32 x 64] as it lies; both are read
//           back as one 16-byte LDS read per operand and step, the up read a broadcast within each group of sixteen lanes
//   inner   for j ascending: sixteen fmaf on registers.  The loop runs to the chunk's true length: no padded step is executed, so
//           not even the sign of a zero depends on the chunking
// Which element is computed by which lane never changes what is computed: every element sees its own chain only.  16-byte (fp32)
// or 8-byte (fp16) accesses of base and out when K % 4 == 0 and both are 16-byte aligned, else element-wise accesses of the same
// elements.  No atomics, no data-dependent addressing, no inline assembly.
#include <stdint.h>

#include "vd_common.h"
#include "../../include/vd_hip.h"

// every operation below is the one the contract names: nothing is fused or re-associated that the source does not spell out
// (build.py compiles this file with -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace {

constexpr int LORA_TILE = 64;         // rows and columns of out per block
constexpr int LORA_THREADS = 256;
constexpr int LORA_RC = 32;           // rank chunk
constexpr int LORA_UP_LD = LORA_TILE + 4;
constexpr int LORA_MAX_TERMS = 8;
constexpr int LORA_MAX_RANK = 256;

struct LoraTerms {                    // passed by value in the kernel arguments
    VdLoraTerm t[LORA_MAX_TERMS];
};

// fp32 -> fp16, to nearest even, in integer arithmetic (apg.hip's apg_round_f16): a rounding of its own.  Left to the compiler, the
// conversion is folded into the fma in front of it (v_fma_mixlo_f16), which rounds the exact result once to fp16.
__device__ __forceinline__ f16 lora_round_f16(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    uint32_t r;
    if (a > 0x7f800000u) {
        r = 0x7e00u;
    } else if (a >= 0x477ff000u) {          // 65520 and above (infinity included): infinity
        r = 0x7c00u;
    } else if (a >= 0x38800000u) {          // 2^-14 and above: a normal fp16; the carry of the rounding runs into the exponent
        const uint32_t t = a - 0x38000000u;
        r = (t + 0xfffu + ((t >> 13) & 1u)) >> 13;
    } else if (a <= 0x33000000u) {          // up to 2^-25 (the tie goes to the even 0)
        r = 0u;
    } else {                                // an fp16 subnormal: a multiple of 2^-24
        const uint32_t mant = (a & 0x7fffffu) | 0x800000u, shift = 126u - (a >> 23);      // 14 .. 24
        const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        r = mant >> shift;
        if (rem > half || (rem == half && (r & 1u))) ++r;
    }
    return __builtin_bit_cast(f16, (uint16_t)(sign | r));
}

template <bool F16>
__global__ __launch_bounds__(LORA_THREADS) void lora_merge_kernel(const void* base_, void* out_, LoraTerms terms, int n_terms, int N,
                                                                  int K, int vec) {
    __shared__ __attribute__((aligned(16))) float up_s[LORA_RC][LORA_UP_LD];     // [j][row of the tile]
    __shared__ __attribute__((aligned(16))) float down_s[LORA_RC][LORA_TILE];    // [j][column of the tile]
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int n0 = blockIdx.y * LORA_TILE, k0 = blockIdx.x * LORA_TILE;
    const int row0 = n0 + 4 * ty, col0 = k0 + 4 * tx;

    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = row0 + i;
        const size_t off = (size_t)n * (size_t)K + (size_t)col0;
        if (vec && n < N && col0 < K) {     // K % 4 == 0: the four columns are inside together
            if (F16) {
                U2H4 b;
                b.u = *reinterpret_cast<const uint2*>(static_cast<const f16*>(base_) + off);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[i][c] = (float)b.e[c];
            } else {
                const float4 b = *reinterpret_cast<const float4*>(static_cast<const float*>(base_) + off);
                acc[i][0] = b.x; acc[i][1] = b.y; acc[i][2] = b.z; acc[i][3] = b.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float b = 0.f;
                if (n < N && col0 + c < K) b = F16 ? (float)static_cast<const f16*>(base_)[off + c] : static_cast<const float*>(base_)[off + c];
                acc[i][c] = b;
            }
        }
    }

    for (int a = 0; a < n_terms; ++a) {
        const float* up = terms.t[a].up;
        const float* down = terms.t[a].down;
        const float scale = terms.t[a].scale;
        const int r = terms.t[a].r;
        float d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) d[i][c] = 0.f;
        for (int j0 = 0; j0 < r; j0 += LORA_RC) {
            const int rc = min(LORA_RC, r - j0);
            // up[n0 + row][j0 + jj] -> up_s[jj][row]: consecutive lanes read consecutive jj of one row
            for (int idx = tid; idx < LORA_TILE * LORA_RC; idx += LORA_THREADS) {
                const int row = idx / LORA_RC, jj = idx % LORA_RC;
                float v = 0.f;
                if (n0 + row < N && jj < rc) v = up[(size_t)(n0 + row) * (size_t)r + (size_t)(j0 + jj)];
                up_s[jj][row] = v;
            }
            // down[j0 + jj][k0 + c] -> down_s[jj][c]: consecutive lanes read consecutive columns
            for (int idx = tid; idx < LORA_RC * LORA_TILE; idx += LORA_THREADS) {
                const int jj = idx / LORA_TILE, c = idx % LORA_TILE;
                float v = 0.f;
                if (jj < rc && k0 + c < K) v = down[(size_t)(j0 + jj) * (size_t)K + (size_t)(k0 + c)];
                down_s[jj][c] = v;
            }
            __syncthreads();
#pragma unroll 4
            for (int jj = 0; jj < rc; ++jj) {
                const float4 u4 = *reinterpret_cast<const float4*>(&up_s[jj][4 * ty]);
                const float4 w4 = *reinterpret_cast<const float4*>(&down_s[jj][4 * tx]);
                const float u[4] = {u4.x, u4.y, u4.z, u4.w}, w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 4; ++c) d[i][c] = fmaf(u[i], w[c], d[i][c]);
            }
            __syncthreads();        // the next chunk (or term) overwrites the stage
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(scale, d[i][c], acc[i][c]);
    }

#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = row0 + i;
        if (n >= N) continue;
        const size_t off = (size_t)n * (size_t)K + (size_t)col0;
        if (vec && col0 < K) {
            if (F16) {
                U2H4 o;
#pragma unroll
                for (int c = 0; c < 4; ++c) o.e[c] = lora_round_f16(acc[i][c]);
                *reinterpret_cast<uint2*>(static_cast<f16*>(out_) + off) = o.u;
            } else {
                *reinterpret_cast<float4*>(static_cast<float*>(out_) + off) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (col0 + c >= K) continue;
                if (F16) static_cast<f16*>(out_)[off + c] = lora_round_f16(acc[i][c]);
                else static_cast<float*>(out_)[off + c] = acc[i][c];
            }
        }
    }
}

}  // namespace

extern "C" int vd_lora_merge(const void* base, void* out, int out_is_f16, const VdLoraTerm* terms, int n_terms, int N, int K,
                             hipStream_t stream) {
    VD_REQUIRE(base && out && terms, "vd_lora_merge: null pointer");
    VD_REQUIRE(n_terms >= 1 && n_terms <= LORA_MAX_TERMS, "vd_lora_merge: n_terms = %d outside 1..%d", n_terms, LORA_MAX_TERMS);
    VD_REQUIRE(N > 0 && K > 0, "vd_lora_merge: N = %d and K = %d must be positive", N, K);
    VD_REQUIRE((N + LORA_TILE - 1) / LORA_TILE <= 65535, "vd_lora_merge: N = %d exceeds the grid (65535 tiles of %d rows)", N, LORA_TILE);
    const size_t es = out_is_f16 ? 2 : 4, bytes = (size_t)N * (size_t)K * es;
    const uintptr_t b0 = (uintptr_t)base, o0 = (uintptr_t)out;
    VD_REQUIRE(base != out && (b0 + bytes <= o0 || o0 + bytes <= b0), "vd_lora_merge: base and out must not alias (base == out or overlapping)");
    VD_REQUIRE(((b0 | o0) & (es - 1)) == 0, "vd_lora_merge: base and out must be aligned to their element size");
    LoraTerms tt = {};
    for (int a = 0; a < n_terms; ++a) {
        VD_REQUIRE(terms[a].up && terms[a].down, "vd_lora_merge: null up / down pointer in term %d", a);
        VD_REQUIRE(terms[a].r >= 1 && terms[a].r <= LORA_MAX_RANK, "vd_lora_merge: r = %d of term %d outside 1..%d", terms[a].r, a,
                   LORA_MAX_RANK);
        VD_REQUIRE((((uintptr_t)terms[a].up | (uintptr_t)terms[a].down) & 3) == 0, "vd_lora_merge: up / down of term %d must be aligned to 4 bytes", a);
        tt.t[a] = terms[a];
    }
    const int vec = (K % 4 == 0 && vd_aligned16(base) && vd_aligned16(out)) ? 1 : 0;
    const dim3 grid((unsigned)((K + LORA_TILE - 1) / LORA_TILE), (unsigned)((N + LORA_TILE - 1) / LORA_TILE));
    if (out_is_f16) hipLaunchKernelGGL(lora_merge_kernel<true>, grid, dim3(LORA_THREADS), 0, stream, base, out, tt, n_terms, N, K, vec);
    else hipLaunchKernelGGL(lora_merge_kernel<false>, grid, dim3(LORA_THREADS), 0, stream, base, out, tt, n_terms, N, K, vec);
    return vd_check_launch("vd_lora_merge");
}
