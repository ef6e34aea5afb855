// Seeded noise made where it is used (gfx950): a counter-based Philox4x32-10 generator with a Box-Muller normal map, the
// kernel that fills a tensor with it, and the SDE variant of the fused CFG + DPM-Solver++(2M) update, which adds its noise
// term in place.  Contract (key, counter, normal map): include/vd_hip.h.
// Built with -fno-slp-vectorize (build.py): the packed-fp32 forms of the unrolled 8-element update want every step scalar
// duplicated into a scalar register pair per use, which on top of the inlined logf / sincospif spills scalar registers.
#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

inline int grid_for(size_t n, int per_block = 256, int cap = 8192) {
    size_t g = (n + per_block - 1) / per_block;
    if (g > (size_t)cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

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

// The per-element CFG combine + DPM-Solver++(2M) update of cfg_dpmpp_dev_kernel (elementwise.hip: dpmpp_elem), with its
// roundings written out instead of left to -ffp-contract=fast, so that they do not depend on the loop an element is handled by:
//   e = eu + s (ec - eu);  x0 = (x - sqrt_1mat e) rsqrt_at;  D = w_cur x0 + w_prev h;  x_next = ratio x + c_d D
// SPLIT = false: every product-sum is one fma -- what the 2M kernel's 16-byte loop is compiled to, and the form of every
// element that gets noise.  SPLIT = true: the two products of D and of x_next are rounded before they are added -- what the
// 2M kernel's scalar loop is compiled to, its products paired into packed multiplies; written here as the same packed
// multiplies (a scalar product feeding an add would be fused whatever the source says).  Used only by the scalar loop at
// coef[7] == 0, where this kernel has to give the 2M kernel's bits.
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <bool SPLIT>
__device__ __forceinline__ float dpmpp_elem_exact(float x, float eu, float ec, float h, int guided, bool second, float s,
                                                  float rsqrt_at, float sqrt_1mat, float ratio, float c_d, float w_cur,
                                                  float w_prev, float& x0) {
    const float e = guided ? fmaf(s, ec - eu, eu) : eu;
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

// The 2M update plus coef[7] z, the SDE variant of DPM-Solver++(2M) (dpm_solver.dpmpp_sde_coef_table): z is made in place from
// seeds[i / per_sample] and the element index i % per_sample, with rng = {draw, stream} in device memory (refreshed between
// graph replays like coef).  coef[7] == 0 (uniform over the grid) generates nothing and walks the elements exactly as the 2M
// kernel does, so it gives that kernel's bits.  VEC: every pointer is 16-byte aligned (the host checks); then elements
// [0, n/8*8) move as 8 x fp16 per lane, as in the 2M kernel -- with noise only if per_sample % 8 == 0, so that the 8 elements of
// a lane lie in one sample and take two Philox blocks.  Every other element goes through the scalar loop, which picks its
// normal out of its block by the same functions: the same bits for the same (sample, element) on either path.
template <bool VEC>
__global__ void cfg_dpmpp_sde_dev_kernel(const f16* x, const f16* eps, float* x0_hist, f16* x_next, f16* pred_x0, size_t n,
                                         size_t per_sample, int guided, const float* coef, const int64_t* seeds,
                                         const int* rng) {
    const float s = coef[0], rsqrt_at = coef[1], sqrt_1mat = coef[2], ratio = coef[3], c_d = coef[4], w_cur = coef[5],
                w_prev = coef[6], c_z = coef[7];
    const bool second = w_prev != 0.f;          // uniform over the grid
    const bool noisy = c_z != 0.f;              // uniform over the grid
    const uint32_t draw = (uint32_t)rng[0], stream = (uint32_t)rng[1];
    const f16* eps_c = eps + n;
    // with noise the lane's group index is divided in 32 bits: groups of 8 per sample, and n / 8 must fit one word
    const bool lanes8 = VEC && (!noisy || (per_sample % 8 == 0 && n / 8 <= 0xffffffffull));
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
        if (noisy) {
            const uint32_t g = (uint32_t)(per_sample >> 3), b = (uint32_t)i / g, j = 2u * ((uint32_t)i - b * g);
            const PhiloxKey key = philox_key(seeds, b);
            philox_normal4(key, j, draw, stream, z);
            philox_normal4(key, j + 1u, draw, stream, z + 4);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float xn = dpmpp_elem_exact<false>((float)xv.e[j], (float)eu.e[j], guided ? (float)ec.e[j] : 0.f, h[j], guided,
                                               second, s, rsqrt_at, sqrt_1mat, ratio, c_d, w_cur, w_prev, x0[j]);
            if (noisy) xn = fmaf(c_z, z[j], xn);
            xo.e[j] = (f16)xn;
            po.e[j] = (f16)x0[j];
        }
        reinterpret_cast<uint4*>(x_next)[i] = xo.u;
        hp[0] = make_float4(x0[0], x0[1], x0[2], x0[3]);
        hp[1] = make_float4(x0[4], x0[5], x0[6], x0[7]);
        if (pred_x0 != nullptr) reinterpret_cast<uint4*>(pred_x0)[i] = po.u;
    }
    for (size_t i = nv * 8 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float xf = (float)x[i], euf = (float)eps[i], ecf = guided ? (float)eps_c[i] : 0.f, hf = second ? x0_hist[i] : 0.f;
        float x0, xn;
        if (noisy) {
            const size_t b = i / per_sample;
            xn = dpmpp_elem_exact<false>(xf, euf, ecf, hf, guided, second, s, rsqrt_at, sqrt_1mat, ratio, c_d, w_cur, w_prev, x0);
            xn = fmaf(c_z, philox_normal1(philox_key(seeds, b), i - b * per_sample, draw, stream), xn);
        } else {
            xn = dpmpp_elem_exact<true>(xf, euf, ecf, hf, guided, second, s, rsqrt_at, sqrt_1mat, ratio, c_d, w_cur, w_prev, x0);
        }
        x_next[i] = (f16)xn;
        x0_hist[i] = x0;
        if (pred_x0 != nullptr) pred_x0[i] = (f16)x0;
    }
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

extern "C" int vd_cfg_dpmpp_sde_step_dev_f16(const void* x, const void* eps, float* x0_hist, void* x_next, void* pred_x0,
                                             int64_t n, int64_t per_sample, int guided, const float* coef,
                                             const int64_t* seeds, const int* rng, hipStream_t stream) {
    VD_REQUIRE(x && eps && x0_hist && x_next && coef && seeds && rng && n > 0 && per_sample > 0,
               "vd_cfg_dpmpp_sde_step_dev_f16: bad arguments");
    VD_REQUIRE(n % per_sample == 0, "vd_cfg_dpmpp_sde_step_dev_f16: n = %lld is not a multiple of per_sample = %lld",
               (long long)n, (long long)per_sample);
    VD_REQUIRE((per_sample + 3) / 4 <= (int64_t)1 << 32,
               "vd_cfg_dpmpp_sde_step_dev_f16: per_sample %lld exceeds the 32-bit block counter", (long long)per_sample);
    auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    // the 2M kernel's alignment rule; whether a noisy step can use the 16-byte lanes (per_sample % 8 == 0) is the kernel's call
    const int vec = a16(x) && a16(eps) && (!guided || a16((const f16*)eps + n)) && a16(x0_hist) &&
                    a16(x_next) && (pred_x0 == nullptr || a16(pred_x0));
    const size_t work = vec && per_sample % 8 == 0 ? (size_t)(n + 7) / 8 : (size_t)n;
    if (vec)
        hipLaunchKernelGGL(cfg_dpmpp_sde_dev_kernel<true>, dim3(grid_for(work)), dim3(256), 0, stream, (const f16*)x,
                           (const f16*)eps, x0_hist, (f16*)x_next, (f16*)pred_x0, (size_t)n, (size_t)per_sample, guided, coef,
                           seeds, rng);
    else
        hipLaunchKernelGGL(cfg_dpmpp_sde_dev_kernel<false>, dim3(grid_for(work)), dim3(256), 0, stream, (const f16*)x,
                           (const f16*)eps, x0_hist, (f16*)x_next, (f16*)pred_x0, (size_t)n, (size_t)per_sample, guided, coef,
                           seeds, rng);
    return vd_check_launch("vd_cfg_dpmpp_sde_step_dev_f16");
}
