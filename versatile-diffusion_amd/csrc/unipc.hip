// The fused CFG combine + UniPC (variant bh2, data prediction) corrector + predictor update of one sampling step (gfx950): one
// elementwise kernel, step scalars in device memory, so one captured graph serves every step.  Contract (row layout, which
// operands are read, the roundings): include/vd_hip.h; the rows: lib/model_zoo/unipc.unipc_coef_table.
// Built with -fno-slp-vectorize like noise.hip (build.py): the unrolled 8-element update would otherwise be packed into
// two-wide fp32 forms that want every step scalar duplicated into a scalar register pair.  The roundings are written out
// (unipc_elem), so the flag decides registers, not bits.
#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

// fp32 -> fp16 as a rounding of its own: left to the compiler, a conversion that follows an fma whose operand was widened from
// fp16 is folded into it (v_fma_mixlo_f16), which rounds the exact sum once to fp16.  The empty asm keeps the fp32 value apart.
__device__ __forceinline__ f16 unipc_round_f16(float v) {
    asm("" : "+v"(v));
    return (f16)v;
}

// A row of the step table, read once per lane (uniform over the grid: every branch on it is a scalar branch).
struct UniPCRow {
    float s, rsqrt_at, sqrt_1mat;       // guidance scale, 1/al_t, sg_t
    bool corr;                          // the corrector runs (x_last is read)
    int hist;                           // valid history entries m_1..m_hist before this step, 0..3
    float c_x, c_1, c_2, c_3, c_t;      // x_c    = c_x x_last + c_1 m_1 + c_2 m_2 + c_3 m_3 + c_t m_t
    float p_x, p_t, p_1, p_2;           // x_next = p_x x_c + p_t m_t + p_1 m_1 + p_2 m_2
};

__device__ __forceinline__ UniPCRow unipc_row(const float* coef) {
    UniPCRow r;
    r.s = coef[0]; r.rsqrt_at = coef[1]; r.sqrt_1mat = coef[2];
    r.corr = coef[3] != 0.f;
    r.c_x = coef[4]; r.c_1 = coef[5]; r.c_2 = coef[6]; r.c_3 = coef[7]; r.c_t = coef[8];
    r.p_x = coef[9]; r.p_t = coef[10]; r.p_1 = coef[11]; r.p_2 = coef[12];
    const float h = coef[13];
    r.hist = h >= 3.f ? 3 : h >= 2.f ? 2 : h >= 1.f ? 1 : 0;
    return r;
}

// One element, every rounding written out (the ABI's rule): each product-sum is one fma, in this order, and a term whose
// coefficient is zero is left out (its operand may be uninitialised).  Both loops of the kernel call this, so an element has the
// same bits on either.  RESCALE: e' = k e, one multiply right after e.
template <bool RESCALE>
__device__ __forceinline__ float unipc_elem(const UniPCRow& r, int guided, float x, float eu, float ec, float xl, float m1,
                                            float m2, float m3, float k, float& mt, float& xc) {
    const float eg = guided ? fmaf(r.s, ec - eu, eu) : eu;
    const float e = RESCALE ? k * eg : eg;
    mt = fmaf(-r.sqrt_1mat, e, x) * r.rsqrt_at;
    if (r.corr) {
        float acc = r.c_t * mt;
        if (r.c_1 != 0.f) acc = fmaf(r.c_1, m1, acc);
        if (r.c_2 != 0.f) acc = fmaf(r.c_2, m2, acc);
        if (r.c_3 != 0.f) acc = fmaf(r.c_3, m3, acc);
        xc = fmaf(r.c_x, xl, acc);
    } else {
        xc = x;
    }
    float acc = r.p_t * mt;
    if (r.p_1 != 0.f) acc = fmaf(r.p_1, m1, acc);
    if (r.p_2 != 0.f) acc = fmaf(r.p_2, m2, acc);
    return fmaf(r.p_x, xc, acc);
}

__device__ __forceinline__ void ld8(const float* p, size_t i, float v[8]) {
    const float4 a = reinterpret_cast<const float4*>(p)[2 * i], b = reinterpret_cast<const float4*>(p)[2 * i + 1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void st8(float* p, size_t i, const float v[8]) {
    reinterpret_cast<float4*>(p)[2 * i] = make_float4(v[0], v[1], v[2], v[3]);
    reinterpret_cast<float4*>(p)[2 * i + 1] = make_float4(v[4], v[5], v[6], v[7]);
}

// the guidance rescale of a step: kfac[i / per_sample] multiplies the guided prediction of element i.  Empty without it.
template <bool RESCALE> struct UniPCRescale {};
template <> struct UniPCRescale<true> { const float* kfac; size_t per_sample; };

// Which state is read: x_last only with the corrector on; m_1 when hist >= 1, m_2 when hist >= 2 (a non-zero coefficient
// implies it; the history shift needs them too); m_3 only when c_3 != 0.  A row with hist == 0 (the first step of a call) reads
// no state at all and writes m_1 = m_2 = m_3 = m_t, so after any step every state buffer holds defined values.
// Then x_last = x_c and (m_1, m_2, m_3) = (m_t, m_1, m_2).  x_next may alias x (an element is read and written by one lane).
// VEC: every pointer is 16-byte aligned (the host checks); elements [0, n/8*8) move as 8 x fp16 / 2 x float4 per lane, the rest
// and every element of a misaligned call go through the scalar loop.
template <bool VEC, bool RESCALE>
__global__ void cfg_unipc_dev_kernel(const f16* x, const f16* eps, float* x_last, float* m1, float* m2, float* m3, f16* x_next,
                                     f16* pred_x0, size_t n, int guided, const float* coef, UniPCRescale<RESCALE> rs) {
    const UniPCRow r = unipc_row(coef);
    const bool rd1 = r.hist >= 1, rd2 = r.hist >= 2, rd3 = r.corr && r.c_3 != 0.f;
    const f16* eps_c = eps + n;
    const size_t nv = VEC ? n / 8 : 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
        U4H8 xv, eu, ec, xo, po;
        xv.u = reinterpret_cast<const uint4*>(x)[i];
        eu.u = reinterpret_cast<const uint4*>(eps)[i];
        if (guided) ec.u = reinterpret_cast<const uint4*>(eps_c)[i];
        float xl[8], a1[8], a2[8], a3[8], mt[8], xc[8], kf[8], n2[8], n3[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xl[j] = a1[j] = a2[j] = a3[j] = 0.f;
        if (r.corr) ld8(x_last, i, xl);
        if (rd1) ld8(m1, i, a1);
        if (rd2) ld8(m2, i, a2);
        if (rd3) ld8(m3, i, a3);
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
            const float xn = unipc_elem<RESCALE>(r, guided, (float)xv.e[j], (float)eu.e[j], guided ? (float)ec.e[j] : 0.f, xl[j],
                                                 a1[j], a2[j], a3[j], RESCALE ? kf[j] : 1.f, mt[j], xc[j]);
            xo.e[j] = unipc_round_f16(xn);
            po.e[j] = unipc_round_f16(mt[j]);
            n2[j] = rd1 ? a1[j] : mt[j];
            n3[j] = rd2 ? a2[j] : mt[j];
        }
        reinterpret_cast<uint4*>(x_next)[i] = xo.u;
        if (pred_x0 != nullptr) reinterpret_cast<uint4*>(pred_x0)[i] = po.u;
        st8(x_last, i, xc);
        st8(m3, i, n3);
        st8(m2, i, n2);
        st8(m1, i, mt);
    }
    for (size_t i = nv * 8 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float xf = (float)x[i], euf = (float)eps[i], ecf = guided ? (float)eps_c[i] : 0.f;
        const float xl = r.corr ? x_last[i] : 0.f, a1 = rd1 ? m1[i] : 0.f, a2 = rd2 ? m2[i] : 0.f, a3 = rd3 ? m3[i] : 0.f;
        float k = 1.f, mt, xc;
        if constexpr (RESCALE) k = rs.kfac[i / rs.per_sample];
        const float xn = unipc_elem<RESCALE>(r, guided, xf, euf, ecf, xl, a1, a2, a3, k, mt, xc);
        x_next[i] = unipc_round_f16(xn);
        if (pred_x0 != nullptr) pred_x0[i] = unipc_round_f16(mt);
        x_last[i] = xc;
        m3[i] = rd2 ? a2 : mt;
        m2[i] = rd1 ? a1 : mt;
        m1[i] = mt;
    }
}

// The alignment rule of the other fused updates: 16-byte lanes only when every stream (both eps halves included) is aligned.
template <bool RESCALE>
void launch_unipc(const void* x, const void* eps, float* x_last, float* m1, float* m2, float* m3, void* x_next, void* pred_x0,
                  int64_t n, int guided, const float* coef, UniPCRescale<RESCALE> rs, hipStream_t stream) {
    const bool vec = vd_aligned16(x) && vd_aligned16(eps) && (!guided || vd_aligned16((const f16*)eps + n)) &&
                     vd_aligned16(x_last) && vd_aligned16(m1) && vd_aligned16(m2) && vd_aligned16(m3) &&
                     vd_aligned16(x_next) && (pred_x0 == nullptr || vd_aligned16(pred_x0));
    const int grid = grid_for(vec ? (size_t)(n + 7) / 8 : (size_t)n);
    if (vec)
        hipLaunchKernelGGL((cfg_unipc_dev_kernel<true, RESCALE>), dim3(grid), dim3(256), 0, stream, (const f16*)x,
                           (const f16*)eps, x_last, m1, m2, m3, (f16*)x_next, (f16*)pred_x0, (size_t)n, guided, coef, rs);
    else
        hipLaunchKernelGGL((cfg_unipc_dev_kernel<false, RESCALE>), dim3(grid), dim3(256), 0, stream, (const f16*)x,
                           (const f16*)eps, x_last, m1, m2, m3, (f16*)x_next, (f16*)pred_x0, (size_t)n, guided, coef, rs);
}

// the four state buffers are read and rewritten element by element: two of them sharing memory would make a step read values
// it has already overwritten
bool unipc_state_distinct(const float* a, const float* b, const float* c, const float* d) {
    return a != b && a != c && a != d && b != c && b != d && c != d;
}

}  // namespace

extern "C" int vd_cfg_unipc_step_dev_f16(const void* x, const void* eps, float* x_last, float* m1, float* m2, float* m3,
                                         void* x_next, void* pred_x0, int64_t n, int guided, const float* coef,
                                         hipStream_t stream) {
    VD_REQUIRE(x && eps && x_last && m1 && m2 && m3 && x_next && coef && n > 0, "vd_cfg_unipc_step_dev_f16: bad arguments");
    VD_REQUIRE(unipc_state_distinct(x_last, m1, m2, m3), "vd_cfg_unipc_step_dev_f16: x_last, m1, m2, m3 must be four buffers");
    launch_unipc<false>(x, eps, x_last, m1, m2, m3, x_next, pred_x0, n, guided, coef, UniPCRescale<false>{}, stream);
    return vd_check_launch("vd_cfg_unipc_step_dev_f16");
}

extern "C" int vd_cfg_unipc_step_dev_rs_f16(const void* x, const void* eps, float* x_last, float* m1, float* m2, float* m3,
                                            void* x_next, void* pred_x0, int64_t n, int64_t per_sample, int guided,
                                            const float* coef, const float* kfac, hipStream_t stream) {
    VD_REQUIRE(x && eps && x_last && m1 && m2 && m3 && x_next && coef && n > 0, "vd_cfg_unipc_step_dev_rs_f16: bad arguments");
    VD_REQUIRE(unipc_state_distinct(x_last, m1, m2, m3),
               "vd_cfg_unipc_step_dev_rs_f16: x_last, m1, m2, m3 must be four buffers");
    if (const int rc = vd_rescale_args_ok("vd_cfg_unipc_step_dev_rs_f16", n, per_sample, guided, kfac)) return rc;
    launch_unipc<true>(x, eps, x_last, m1, m2, m3, x_next, pred_x0, n, guided, coef,
                       UniPCRescale<true>{kfac, (size_t)per_sample}, stream);
    return vd_check_launch("vd_cfg_unipc_step_dev_rs_f16");
}
