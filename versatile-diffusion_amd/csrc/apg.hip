// Adaptive projected guidance (Sadat, Hilliges, Weber 2024; diffusers' AdaptiveProjectedGuidance) on gfx950: the fold it adds to a
// step.  Contract (operands, the written-out roundings): include/vd_hip.h.
//
// vd_apg_fold_f16 rewrites replica 0 of the step's eps batch so that every existing fused update (and the guidance-rescale factor
// kernel) runs on the pair unchanged.  One launch; a sample is always handled by ONE block of 1024 lanes, whatever the batch:
//   pass 1  lane t takes the groups of 8 elements t, t + 1024, ... of the sample in order, then element 8 (m / 8) + t of the last
//           partial group: forms D_c and v, stores v, adds v^2, v D_c and D_c^2 to three fp64 sums (an fp32 product is exact there);
//           a fixed butterfly over the wave, then the sixteen waves' sums added in wave order by lane 0, which forms k, p, q
//   pass 2  behind the block barrier the SAME lane walks the SAME elements: reads back its own v, forms D_c again (the same
//           operations on the same operands: the same bits) and writes e_u'
// Which lane adds which element in which order depends on nothing but m, so a sample's outputs have the same bits wherever it
// runs; the 16-byte accesses (x, both replicas and v of THIS sample 16-byte aligned, uniform over the block) and the element-wise
// ones touch the same elements with the same arithmetic.  No atomics, no inline assembly.
#include <stdint.h>

#include "vd_common.h"
#include "../../include/vd_hip.h"

// every operation below is the one the contract names: nothing is fused or re-associated that the source does not spell out
#pragma clang fp contract(off)

namespace {

constexpr int APG_THREADS = 1024;
constexpr int APG_WAVES = APG_THREADS / 64;

// fp32 -> fp16, to nearest even, in integer arithmetic: a rounding of its own.  Left to the compiler, the conversion is folded into
// the fma in front of it (v_fma_mixlo_f16), which rounds the exact result once to fp16.  NaN gives the quiet NaN of its sign.
__device__ __forceinline__ f16 apg_round_f16(float f) {
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

__device__ __forceinline__ double apg_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct ApgCoef {
    float s1, isa, ig, beta, ng32;      // ng32 = -(s1 * isa), the product rounded once
};

__device__ __forceinline__ float apg_dc(float x, float ec, const ApgCoef& c) { return fmaf(-c.s1, ec, x) * c.isa; }

struct ApgSums {
    double vv = 0.0, vd = 0.0, dd = 0.0;
    // returns v, the running direction of this element
    __device__ __forceinline__ float add(float x, float eu, float ec, float vprev, bool mom, const ApgCoef& c) {
        const float D = apg_dc(x, ec, c);
        const float dD = c.ng32 * (ec - eu);
        const float v = mom ? fmaf(c.beta, vprev, dD) : dD;
        const double v64 = (double)v, D64 = (double)D;
        vv += v64 * v64;
        vd += v64 * D64;
        dd += D64 * D64;
        return v;
    }
};

__device__ __forceinline__ f16 apg_out(float x, float ec, float v, float k, float q, const ApgCoef& c) {
    const float D = apg_dc(x, ec, c);
    const float kv = k * v;
    const float nn = fmaf(-q, D, kv);
    return apg_round_f16(fmaf(nn, c.ig, ec));
}

union U8F {
    float4 q[2];
    float e[8];
};

__global__ __launch_bounds__(APG_THREADS) void apg_fold_kernel(const f16* x, f16* eps, float* v, const float* coef, float* fac,
                                                              size_t n, size_t m) {
    __shared__ double part[3][APG_WAVES];
    __shared__ float kq[2];
    ApgCoef c;
    c.s1 = coef[0];
    c.isa = coef[1];
    c.ig = coef[2];
    c.beta = coef[3];
    c.ng32 = -(c.s1 * c.isa);
    const float r = coef[4], ome = coef[5];
    const bool mom = c.beta != 0.f;     // beta_eff == 0: the state is not read
    const size_t B = n / m, groups = m / 8;
    const int tid = threadIdx.x, wave = tid >> 6;
    for (size_t b = blockIdx.x; b < B; b += gridDim.x) {
        const f16* xs = x + b * m;
        f16* eu = eps + b * m;
        const f16* ec = eu + n;
        float* vs = v + b * m;
        const bool vec = (((uintptr_t)xs | (uintptr_t)eu | (uintptr_t)ec | (uintptr_t)vs) & 15) == 0;
        const size_t t = 8 * groups + (size_t)tid;      // this lane's element of the last partial group, if t < m
        ApgSums acc;
        for (size_t g = tid; g < groups; g += APG_THREADS) {
            U4H8 ux, uu, uc;
            U8F uv;
            if (vec) {
                ux.u = reinterpret_cast<const uint4*>(xs)[g];
                uu.u = reinterpret_cast<const uint4*>(eu)[g];
                uc.u = reinterpret_cast<const uint4*>(ec)[g];
                if (mom) {
                    uv.q[0] = reinterpret_cast<const float4*>(vs)[2 * g];
                    uv.q[1] = reinterpret_cast<const float4*>(vs)[2 * g + 1];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    ux.e[j] = xs[8 * g + j];
                    uu.e[j] = eu[8 * g + j];
                    uc.e[j] = ec[8 * g + j];
                    if (mom) uv.e[j] = vs[8 * g + j];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                uv.e[j] = acc.add((float)ux.e[j], (float)uu.e[j], (float)uc.e[j], mom ? uv.e[j] : 0.f, mom, c);
            if (vec) {
                reinterpret_cast<float4*>(vs)[2 * g] = uv.q[0];
                reinterpret_cast<float4*>(vs)[2 * g + 1] = uv.q[1];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) vs[8 * g + j] = uv.e[j];
            }
        }
        if (t < m) vs[t] = acc.add((float)xs[t], (float)eu[t], (float)ec[t], mom ? vs[t] : 0.f, mom, c);
        const double w[3] = {apg_wave_sum(acc.vv), apg_wave_sum(acc.vd), apg_wave_sum(acc.dd)};
        if ((tid & 63) == 0) {
#pragma unroll
            for (int s = 0; s < 3; ++s) part[s][wave] = w[s];
        }
        __syncthreads();
        if (tid == 0) {
            double tot[3];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                double a = part[s][0];
#pragma unroll
                for (int i = 1; i < APG_WAVES; ++i) a += part[s][i];
                tot[s] = a;
            }
            const double nv = sqrt(tot[0]), rd = (double)r;
            double k = 1.0;
            if (rd != 0.0 && nv != 0.0) k = fmin(1.0, rd / nv);
            const double p = tot[2] == 0.0 ? 0.0 : k * tot[1] / tot[2];
            const double q = (double)ome * p;
            fac[4 * b + 0] = (float)nv;
            fac[4 * b + 1] = (float)k;
            fac[4 * b + 2] = (float)p;
            fac[4 * b + 3] = (float)sqrt(tot[2]);
            kq[0] = (float)k;
            kq[1] = (float)q;
        }
        __syncthreads();
        const float k = kq[0], q = kq[1];
        for (size_t g = tid; g < groups; g += APG_THREADS) {
            U4H8 ux, uc, uo;
            U8F uv;
            if (vec) {
                ux.u = reinterpret_cast<const uint4*>(xs)[g];
                uc.u = reinterpret_cast<const uint4*>(ec)[g];
                uv.q[0] = reinterpret_cast<const float4*>(vs)[2 * g];
                uv.q[1] = reinterpret_cast<const float4*>(vs)[2 * g + 1];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    ux.e[j] = xs[8 * g + j];
                    uc.e[j] = ec[8 * g + j];
                    uv.e[j] = vs[8 * g + j];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) uo.e[j] = apg_out((float)ux.e[j], (float)uc.e[j], uv.e[j], k, q, c);
            if (vec) {
                reinterpret_cast<uint4*>(eu)[g] = uo.u;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) eu[8 * g + j] = uo.e[j];
            }
        }
        if (t < m) eu[t] = apg_out((float)xs[t], (float)ec[t], vs[t], k, q, c);
        __syncthreads();        // part / kq are reused by the block's next sample
    }
}

}  // namespace

extern "C" int vd_apg_fold_f16(const void* x, void* eps, float* v, const float* coef, float* fac, int64_t n, int64_t per_sample,
                               hipStream_t stream) {
    VD_REQUIRE(x && eps && v && coef && fac, "vd_apg_fold_f16: null pointer");
    VD_REQUIRE(n > 0 && per_sample > 0, "vd_apg_fold_f16: n = %lld and per_sample = %lld must be positive", (long long)n,
               (long long)per_sample);
    VD_REQUIRE(n % per_sample == 0, "vd_apg_fold_f16: n = %lld is not a multiple of per_sample = %lld", (long long)n,
               (long long)per_sample);
    VD_REQUIRE((((uintptr_t)x | (uintptr_t)eps) & 1) == 0 && (((uintptr_t)v | (uintptr_t)coef | (uintptr_t)fac) & 3) == 0,
               "vd_apg_fold_f16: x, eps, v, coef and fac must be aligned to their element size");
    const int64_t B = n / per_sample;
    hipLaunchKernelGGL(apg_fold_kernel, dim3((unsigned)(B < 65536 ? B : 65536)), dim3(APG_THREADS), 0, stream, (const f16*)x,
                       (f16*)eps, v, coef, fac, (size_t)n, (size_t)per_sample);
    return vd_check_launch("vd_apg_fold_f16");
}
