// Seeded noise made where it is used (gfx950): a counter-based Philox4x32-10 generator with a Box-Muller normal map, the
// kernel that fills a tensor with it, and the fused CFG + DPM-Solver++(2M) update: one kernel, instantiated without noise (the
// 2M sampler) and with its noise term added in place (the SDE variant).  Contract (key, counter, normal map, the update's
// roundings): include/vd_hip.h.
// Built with -fno-slp-vectorize (build.py): the packed-fp32 forms of the unrolled 8-element update want every step scalar
// duplicated into a scalar register pair per use, which on top of the inlined logf / sincospif spills scalar registers.  The
// update's roundings are written out (dpmpp_elem_exact), so the flag decides registers, not bits.
#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123) in plain integer
// arithmetic: a counter-based generator, so the noise of (sample, draw, element) is a pure function of the sample's seed and
// needs neither a table nor a generator state.  Key / counter layout and the normal map: include/vd_hip.h.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t r[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// Box-Muller on two words: u = ((r >> 9) + 0.5) 2^-23 is exact in fp32 and lies in (0, 1); accurate logf / sincospif
// (sin and cos of pi * (2 u2): the argument 2 u2 is exact, so the angle is never rounded)
__device__ __forceinline__ void philox_normal_pair(uint32_t r_even, uint32_t r_odd, float& z_even, float& z_odd) {
    const float u1 = ((float)(r_even >> 9) + 0.5f) * 0x1p-23f, u2 = ((float)(r_odd >> 9) + 0.5f) * 0x1p-23f;
    const float rad = sqrtf(-2.f * logf(u1));
    float s, c;
    sincospif(2.f * u2, &s, &c);
    z_even = rad * c;
    z_odd = rad * s;
}

// A sample's key (low word, high word of its seed), read as two words: on a 64-bit seed register the compiler does the ten
// key bumps as 64-bit additions with one scalar register pair per round constant.
struct PhiloxKey { uint32_t lo, hi; };
__device__ __forceinline__ PhiloxKey philox_key(const int64_t* seeds, size_t b) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(seeds + b);
    return PhiloxKey{w[0], w[1]};
}

// the four normals of elements 4j .. 4j+3 of the sample with this key
__device__ __forceinline__ void philox_normal4(PhiloxKey key, uint32_t j, uint32_t draw, uint32_t stream, float z[4]) {
    uint32_t r[4];
    philox4x32_10(j, 0u, draw, stream, key.lo, key.hi, r);
    philox_normal_pair(r[0], r[1], z[0], z[1]);
    philox_normal_pair(r[2], r[3], z[2], z[3]);
}

// the normal of element e alone (scalar paths): the same words through the same pair function, so the same bits
__device__ __forceinline__ float philox_normal1(PhiloxKey key, size_t e, uint32_t draw, uint32_t stream) {
    uint32_t r[4];
    philox4x32_10((uint32_t)(e >> 2), 0u, draw, stream, key.lo, key.hi, r);
    float z_even, z_odd;
    const bool hi = (e & 2) != 0;
    philox_normal_pair(hi ? r[2] : r[0], hi ? r[3] : r[1], z_even, z_odd);
    return (e & 1) ? z_odd : z_even;
}

// out[b, e] = scale z(seeds[b], e): one lane per block of four elements, the last block of a sample may be partial
template <typename T>
__global__ void philox_normal_kernel(const int64_t* seeds, T* out, int B, size_t per_sample, uint32_t draw, uint32_t stream,
                                     float scale) {
    const size_t nblk = (per_sample + 3) / 4, total = (size_t)B * nblk;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / nblk, j = i - b * nblk;
        float z[4];
        philox_normal4(philox_key(seeds, b), (uint32_t)j, draw, stream, z);
        T* o = out + b * per_sample;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * j + k < per_sample) o[4 * j + k] = (T)(scale * z[k]);
    }
}

// The per-element CFG combine + DPM-Solver++(2M) update, with its roundings written out instead of left to -ffp-contract=fast:
//   e = eu + s (ec - eu);  x0 = (x - sqrt_1mat e) rsqrt_at;  D = w_cur x0 + w_prev h;  x_next = ratio x + c_d D
// SPLIT = false: every product-sum is one fma.  SPLIT = true: the two products of D and of x_next are rounded before they are
// added; written as packed multiplies (a scalar product feeding an add would be fused whatever the source says).  e and x0 are
// fused in both forms.  Which element takes which form: the rule above cfg_dpmpp_dev_kernel.
typedef float f32x2 __attribute__((ext_vector_type(2)));

// RESCALE (guidance rescale, vd_cfg_rescale_factor_f16): e' = k e, one fp32 multiply right after e, takes e's place.
template <bool SPLIT, bool RESCALE = false>
__device__ __forceinline__ float dpmpp_elem_exact(float x, float eu, float ec, float h, int guided, bool second, float s,
                                                  float rsqrt_at, float sqrt_1mat, float ratio, float c_d, float w_cur,
                                                  float w_prev, float& x0, float k = 1.f) {
    const float eg = guided ? fmaf(s, ec - eu, eu) : eu;
    const float e = RESCALE ? k * eg : eg;
    x0 = fmaf(-sqrt_1mat, e, x) * rsqrt_at;
    if (SPLIT) {
        const f32x2 pd = f32x2{w_cur, w_prev} * f32x2{x0, h};
        const float d = second ? pd.x + pd.y : pd.x;
        const f32x2 px = f32x2{ratio, c_d} * f32x2{x, d};
        return px.x + px.y;
    }
    float d = w_cur * x0;
    if (second) d = fmaf(w_prev, h, d);
    return fmaf(ratio, x, c_d * d);
}

// fp32 -> fp16 as a rounding of its own.  Left to the compiler, a conversion that follows an fma whose operand was widened from
// fp16 is folded into it (v_fma_mixlo_f16 / v_fma_mixhi_f16), and that instruction rounds the exact sum once to fp16: other
// bits than the fp32 fma followed by the conversion, in about one output per 10^4.  The empty asm keeps the fp32 value apart.
__device__ __forceinline__ f16 round_f16(float v) {
    asm("" : "+v"(v));
    return (f16)v;
}

// where the noise of a step comes from: seeds[i / per_sample] and rng = {draw, stream} in device memory (refreshed between
// graph replays like coef).  Empty without noise, so those instances take no seeds and hold no generator code.
template <bool NOISE> struct StepNoise {};
template <> struct StepNoise<true> { const int64_t* seeds; const int* rng; size_t per_sample; };

// the guidance rescale of a step: kfac[i / per_sample] multiplies the guided prediction of element i.  Empty without it.
template <bool RESCALE> struct StepRescale {};
template <> struct StepRescale<true> { const float* kfac; size_t per_sample; };

// CFG combine + DPM-Solver++(2M) multistep update, step scalars in device memory (one captured graph serves all steps):
// coef = {guidance scale, 1/sqrt(a_t), sqrt(1 - a_t), sigma_next / sigma_t, c_d, w_cur, w_prev, c_z}, then x0_hist = x0 (fp32).
// w_prev == 0 (first-order rows) never reads x0_hist: it is uninitialised on the first step of a call.  x_next may alias x
// (each element is read and written by the same lane).
// NOISE = false is the 2M update: coef[7] is not read.  NOISE = true adds coef[7] z, the SDE variant of DPM-Solver++(2M)
// (dpm_solver.dpmpp_sde_coef_table), z made in place from the sample's seed and the element index i % per_sample; coef[7] == 0
// (uniform over the grid) generates nothing and walks the elements exactly as NOISE = false does.
// VEC: every pointer is 16-byte aligned (the host checks); then elements [0, n/8*8) move as 8 x fp16 / 2 x float4 per lane --
// with noise only if per_sample % 8 == 0, so that the 8 elements of a lane lie in one sample and take two Philox blocks.  Every
// other element goes through the scalar loop, which picks its normal out of its block by the same functions: the same bits
// for the same (sample, element) on either path.
// Roundings (the ABI's rule, include/vd_hip.h), in terms of dpmpp_elem_exact:
//   elements moved by the 16-byte loop             every product-sum is one fma (SPLIT = false)
//   elements of the scalar loop without noise      the two products of D and of x_next are rounded, then added (SPLIT = true)
//   elements that get noise, on either loop        fused (SPLIT = false), then x_next = fma(c_z, z, x_next)
// and x_next, pred_x0 are those fp32 values rounded to fp16 (round_f16), never a sum rounded straight to fp16.
// RESCALE = true (the _rs entry points): e' = kfac[i / rs.per_sample] * e takes e's place, everything after it as above.  A lane
// of the 16-byte loop whose 8 elements do not lie in one sample (rs.per_sample % 8 != 0) looks the factor up per element.
template <bool VEC, bool NOISE, bool RESCALE>
__global__ void cfg_dpmpp_dev_kernel(const f16* x, const f16* eps, float* x0_hist, f16* x_next, f16* pred_x0, size_t n,
                                     int guided, const float* coef, StepNoise<NOISE> src, StepRescale<RESCALE> rs) {
    const float s = coef[0], rsqrt_at = coef[1], sqrt_1mat = coef[2], ratio = coef[3], c_d = coef[4], w_cur = coef[5],
                w_prev = coef[6];
    const bool second = w_prev != 0.f;          // uniform over the grid
    float c_z = 0.f;
    uint32_t draw = 0, stream = 0;
    bool lanes8 = VEC;
    if constexpr (NOISE) {
        c_z = coef[7];
        draw = (uint32_t)src.rng[0], stream = (uint32_t)src.rng[1];
        // with noise the lane's group index is divided in 32 bits: groups of 8 per sample, and n / 8 must fit one word
        lanes8 = VEC && (c_z == 0.f || (src.per_sample % 8 == 0 && n / 8 <= 0xffffffffull));
    }
    const bool noisy = c_z != 0.f;              // uniform over the grid; false at compile time without NOISE
    const f16* eps_c = eps + n;
    const size_t nv = lanes8 ? n / 8 : 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
        U4H8 xv, eu, ec, xo, po;
        xv.u = reinterpret_cast<const uint4*>(x)[i];
        eu.u = reinterpret_cast<const uint4*>(eps)[i];
        if (guided) ec.u = reinterpret_cast<const uint4*>(eps_c)[i];
        float h[8], x0[8], z[8];
        float4* hp = reinterpret_cast<float4*>(x0_hist) + 2 * i;
        if (second) {
            const float4 h0 = hp[0], h1 = hp[1];
            h[0] = h0.x; h[1] = h0.y; h[2] = h0.z; h[3] = h0.w; h[4] = h1.x; h[5] = h1.y; h[6] = h1.z; h[7] = h1.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = 0.f;
        }
        if constexpr (NOISE) {
            if (noisy) {
                const uint32_t g = (uint32_t)(src.per_sample >> 3), b = (uint32_t)i / g, j = 2u * ((uint32_t)i - b * g);
                const PhiloxKey key = philox_key(src.seeds, b);
                philox_normal4(key, j, draw, stream, z);
                philox_normal4(key, j + 1u, draw, stream, z + 4);
            }
        }
        float kf[8];
        if constexpr (RESCALE) {
            const size_t e0 = 8 * i, b0 = e0 / rs.per_sample;
            if (e0 - b0 * rs.per_sample + 8 <= rs.per_sample) {
                const float k = rs.kfac[b0];
#pragma unroll
                for (int j = 0; j < 8; ++j) kf[j] = k;
            } else {                                    // the lane straddles samples (any number of them: per_sample < 8)
#pragma unroll
                for (int j = 0; j < 8; ++j) kf[j] = rs.kfac[(e0 + j) / rs.per_sample];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float xn = dpmpp_elem_exact<false, RESCALE>((float)xv.e[j], (float)eu.e[j], guided ? (float)ec.e[j] : 0.f, h[j],
                                                        guided, second, s, rsqrt_at, sqrt_1mat, ratio, c_d, w_cur, w_prev,
                                                        x0[j], RESCALE ? kf[j] : 1.f);
            if (noisy) xn = fmaf(c_z, z[j], xn);
            xo.e[j] = round_f16(xn);
            po.e[j] = round_f16(x0[j]);
        }
        reinterpret_cast<uint4*>(x_next)[i] = xo.u;
        hp[0] = make_float4(x0[0], x0[1], x0[2], x0[3]);
        hp[1] = make_float4(x0[4], x0[5], x0[6], x0[7]);
        if (pred_x0 != nullptr) reinterpret_cast<uint4*>(pred_x0)[i] = po.u;
    }
    for (size_t i = nv * 8 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float xf = (float)x[i], euf = (float)eps[i], ecf = guided ? (float)eps_c[i] : 0.f, hf = second ? x0_hist[i] : 0.f;
        float x0, xn, k = 1.f;
        if constexpr (RESCALE) k = rs.kfac[i / rs.per_sample];
        if (!noisy) {
            xn = dpmpp_elem_exact<true, RESCALE>(xf, euf, ecf, hf, guided, second, s, rsqrt_at, sqrt_1mat, ratio, c_d, w_cur,
                                                 w_prev, x0, k);
        } else if constexpr (NOISE) {
            const size_t b = i / src.per_sample;
            xn = dpmpp_elem_exact<false, RESCALE>(xf, euf, ecf, hf, guided, second, s, rsqrt_at, sqrt_1mat, ratio, c_d, w_cur,
                                                  w_prev, x0, k);
            xn = fmaf(c_z, philox_normal1(philox_key(src.seeds, b), i - b * src.per_sample, draw, stream), xn);
        }
        x_next[i] = round_f16(xn);
        x0_hist[i] = x0;
        if (pred_x0 != nullptr) pred_x0[i] = round_f16(x0);
    }
}

// Both entry points' launch.  The alignment rule: 16-byte lanes only when every stream (both eps halves included) is aligned
// (torch slices can start anywhere).  lanes8: a lane of the aligned kernel takes 8 elements (sizes the grid; whether a noisy
// step can use the lanes, per_sample % 8 == 0, is the kernel's call).
template <bool NOISE, bool RESCALE>
void launch_dpmpp(const void* x, const void* eps, float* x0_hist, void* x_next, void* pred_x0, int64_t n, int guided,
                  const float* coef, bool lanes8, StepNoise<NOISE> src, StepRescale<RESCALE> rs, hipStream_t stream) {
    const bool vec = vd_aligned16(x) && vd_aligned16(eps) && (!guided || vd_aligned16((const f16*)eps + n)) &&
                     vd_aligned16(x0_hist) && vd_aligned16(x_next) && (pred_x0 == nullptr || vd_aligned16(pred_x0));
    const int grid = grid_for(vec && lanes8 ? (size_t)(n + 7) / 8 : (size_t)n);
    if (vec)
        hipLaunchKernelGGL((cfg_dpmpp_dev_kernel<true, NOISE, RESCALE>), dim3(grid), dim3(256), 0, stream, (const f16*)x,
                           (const f16*)eps, x0_hist, (f16*)x_next, (f16*)pred_x0, (size_t)n, guided, coef, src, rs);
    else
        hipLaunchKernelGGL((cfg_dpmpp_dev_kernel<false, NOISE, RESCALE>), dim3(grid), dim3(256), 0, stream, (const f16*)x,
                           (const f16*)eps, x0_hist, (f16*)x_next, (f16*)pred_x0, (size_t)n, guided, coef, src, rs);
}

}  // namespace

extern "C" int vd_philox_normal(const int64_t* seeds, void* out, int out_is_f32, int B, int64_t per_sample, int draw,
                                int stream_tag, float scale, hipStream_t stream) {
    VD_REQUIRE(seeds && out && B > 0 && per_sample > 0 && draw >= 0 && stream_tag >= 0, "vd_philox_normal: bad arguments");
    VD_REQUIRE((per_sample + 3) / 4 <= (int64_t)1 << 32, "vd_philox_normal: per_sample %lld exceeds the 32-bit block counter",
               (long long)per_sample);
    const int grid = grid_for((size_t)B * (size_t)((per_sample + 3) / 4));
    if (out_is_f32)
        hipLaunchKernelGGL(philox_normal_kernel<float>, dim3(grid), dim3(256), 0, stream, seeds, (float*)out, B,
                           (size_t)per_sample, (uint32_t)draw, (uint32_t)stream_tag, scale);
    else
        hipLaunchKernelGGL(philox_normal_kernel<f16>, dim3(grid), dim3(256), 0, stream, seeds, (f16*)out, B,
                           (size_t)per_sample, (uint32_t)draw, (uint32_t)stream_tag, scale);
    return vd_check_launch("vd_philox_normal");
}

extern "C" int vd_cfg_dpmpp_step_dev_f16(const void* x, const void* eps, float* x0_hist, void* x_next, void* pred_x0,
                                         int64_t n, int guided, const float* coef, hipStream_t stream) {
    VD_REQUIRE(x && eps && x0_hist && x_next && coef && n > 0, "vd_cfg_dpmpp_step_dev_f16: bad arguments");
    launch_dpmpp<false, false>(x, eps, x0_hist, x_next, pred_x0, n, guided, coef, true, StepNoise<false>{},
                               StepRescale<false>{}, stream);
    return vd_check_launch("vd_cfg_dpmpp_step_dev_f16");
}

extern "C" int vd_cfg_dpmpp_step_dev_rs_f16(const void* x, const void* eps, float* x0_hist, void* x_next, void* pred_x0,
                                            int64_t n, int64_t per_sample, int guided, const float* coef, const float* kfac,
                                            hipStream_t stream) {
    VD_REQUIRE(x && eps && x0_hist && x_next && coef && n > 0, "vd_cfg_dpmpp_step_dev_rs_f16: bad arguments");
    if (const int rc = vd_rescale_args_ok("vd_cfg_dpmpp_step_dev_rs_f16", n, per_sample, guided, kfac)) return rc;
    launch_dpmpp<false, true>(x, eps, x0_hist, x_next, pred_x0, n, guided, coef, true, StepNoise<false>{},
                              StepRescale<true>{kfac, (size_t)per_sample}, stream);
    return vd_check_launch("vd_cfg_dpmpp_step_dev_rs_f16");
}

extern "C" int vd_cfg_dpmpp_sde_step_dev_f16(const void* x, const void* eps, float* x0_hist, void* x_next, void* pred_x0,
                                             int64_t n, int64_t per_sample, int guided, const float* coef,
                                             const int64_t* seeds, const int* rng, hipStream_t stream) {
    VD_REQUIRE(x && eps && x0_hist && x_next && coef && seeds && rng && n > 0 && per_sample > 0,
               "vd_cfg_dpmpp_sde_step_dev_f16: bad arguments");
    VD_REQUIRE(n % per_sample == 0, "vd_cfg_dpmpp_sde_step_dev_f16: n = %lld is not a multiple of per_sample = %lld",
               (long long)n, (long long)per_sample);
    VD_REQUIRE((per_sample + 3) / 4 <= (int64_t)1 << 32,
               "vd_cfg_dpmpp_sde_step_dev_f16: per_sample %lld exceeds the 32-bit block counter", (long long)per_sample);
    launch_dpmpp<true, false>(x, eps, x0_hist, x_next, pred_x0, n, guided, coef, per_sample % 8 == 0,
                              StepNoise<true>{seeds, rng, (size_t)per_sample}, StepRescale<false>{}, stream);
    return vd_check_launch("vd_cfg_dpmpp_sde_step_dev_f16");
}

extern "C" int vd_cfg_dpmpp_sde_step_dev_rs_f16(const void* x, const void* eps, float* x0_hist, void* x_next, void* pred_x0,
                                                int64_t n, int64_t per_sample, int guided, const float* coef,
                                                const int64_t* seeds, const int* rng, const float* kfac, hipStream_t stream) {
    VD_REQUIRE(x && eps && x0_hist && x_next && coef && seeds && rng && n > 0 && per_sample > 0,
               "vd_cfg_dpmpp_sde_step_dev_rs_f16: bad arguments");
    if (const int rc = vd_rescale_args_ok("vd_cfg_dpmpp_sde_step_dev_rs_f16", n, per_sample, guided, kfac)) return rc;
    VD_REQUIRE((per_sample + 3) / 4 <= (int64_t)1 << 32,
               "vd_cfg_dpmpp_sde_step_dev_rs_f16: per_sample %lld exceeds the 32-bit block counter", (long long)per_sample);
    launch_dpmpp<true, true>(x, eps, x0_hist, x_next, pred_x0, n, guided, coef, per_sample % 8 == 0,
                             StepNoise<true>{seeds, rng, (size_t)per_sample}, StepRescale<true>{kfac, (size_t)per_sample},
                             stream);
    return vd_check_launch("vd_cfg_dpmpp_sde_step_dev_rs_f16");
}
