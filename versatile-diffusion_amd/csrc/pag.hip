// Perturbed-attention guidance (Ahn et al. 2024) on gfx950: the two element-wise passes it adds to a step.  Contracts (operands,
// the written-out roundings): include/vd_hip.h.
//
// vd_attention_ident_f16: self-attention whose attention map is the identity for the samples from `ident_from` on.  The samples in
// front of it go through vd_attention_f16 itself (the same kernel instances on a smaller batch: a sample's bits do not depend on
// the batch it sits in); for the others softmax(I) v = v, so the "attention" is ONE copy launch of v's head columns into out, 16
// bytes per lane.  Both are bandwidth-bound: the copy moves 2 * rows * H * D * 2 bytes and nothing else.
//
// vd_pag_fold_f16: folds the perturbed prediction into replica 0 of the step's eps batch so that every existing fused update (and
// the guidance-rescale factor kernel) runs on the leading replicas unchanged.  One read of three (two) replicas, one write of one.
#include <stdio.h>

#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

constexpr int PAG_THREADS = 256;

// fp32 -> fp16 as a rounding of its own (freeu.hip's rule): left to the compiler, the conversion is folded into the fma in front
// of it (v_fma_mixlo_f16), which rounds the exact result once to fp16.  The empty asm keeps the fp32 value.
__device__ __forceinline__ f16 pag_round_f16(float v) {
    asm("" : "+v"(v));
    return (f16)v;
}

// one work item = 8 consecutive columns of one row of one identity sample
__global__ __launch_bounds__(PAG_THREADS) void pag_ident_copy_kernel(const f16* v, f16* out, int N, int chunks, int ldv, int ldo,
                                                                    int64_t sv, int64_t so, size_t work) {
    const size_t stride = (size_t)gridDim.x * PAG_THREADS;
    const size_t per_sample = (size_t)N * chunks;
    for (size_t t = (size_t)blockIdx.x * PAG_THREADS + threadIdx.x; t < work; t += stride) {
        const size_t b = t / per_sample, r = t - b * per_sample;
        const size_t n = r / chunks, c = r - n * chunks;
        const uint4 u = *reinterpret_cast<const uint4*>(v + (int64_t)b * sv + (int64_t)n * ldv + (int64_t)c * 8);
        *reinterpret_cast<uint4*>(out + (int64_t)b * so + (int64_t)n * ldo + (int64_t)c * 8) = u;
    }
}

__device__ __forceinline__ f16 pag_fold_one(f16 a, f16 c, f16 p, float w) {
    const float d = (float)c - (float)p;
    return pag_round_f16(fmaf(w, d, (float)a));
}

// VEC: 8 elements per work item through 16-byte accesses (every replica 16-byte aligned); else one element per work item
template <bool VEC>
__global__ __launch_bounds__(PAG_THREADS) void pag_fold_kernel(f16* eps, int64_t n, int reps, const float* wp) {
    const float w = *wp;
    if (w == 0.f) return;       // nothing to fold: replica 0 keeps its bits (a -0 and a NaN payload included)
    f16* a = eps;
    const f16* c = eps + (int64_t)(reps - 2) * n;
    const f16* p = eps + (int64_t)(reps - 1) * n;
    const size_t stride = (size_t)gridDim.x * PAG_THREADS;
    const size_t work = VEC ? (size_t)(n / 8) : (size_t)n;
    for (size_t t = (size_t)blockIdx.x * PAG_THREADS + threadIdx.x; t < work; t += stride) {
        if constexpr (VEC) {
            U4H8 va, vc, vp;
            va.u = *reinterpret_cast<const uint4*>(a + t * 8);
            vc.u = *reinterpret_cast<const uint4*>(c + t * 8);
            vp.u = *reinterpret_cast<const uint4*>(p + t * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) va.e[j] = pag_fold_one(va.e[j], vc.e[j], vp.e[j], w);
            *reinterpret_cast<uint4*>(a + t * 8) = va.u;
        } else {
            a[t] = pag_fold_one(a[t], c[t], p[t], w);
        }
    }
}

}  // namespace

extern "C" int vd_attention_ident_f16(const void* q, const void* k, const void* v, void* out, int B, int H, int Nq, int Nk, int D,
                                      int ldq, int ldk, int ldv, int ldo, int64_t sq, int64_t sk, int64_t sv, int64_t so,
                                      float scale, int causal, int ident_from, hipStream_t stream) {
    VD_REQUIRE(q && k && v && out, "vd_attention_ident_f16: null pointer");
    VD_REQUIRE(B > 0 && H > 0 && Nq > 0 && Nk > 0 && D > 0, "vd_attention_ident_f16: empty problem B=%d H=%d Nq=%d Nk=%d D=%d", B, H,
               Nq, Nk, D);
    VD_REQUIRE(Nq == Nk, "vd_attention_ident_f16: the identity map needs self-attention, Nq = %d and Nk = %d differ", Nq, Nk);
    VD_REQUIRE(causal == 0, "vd_attention_ident_f16: no causal mask (causal = %d)", causal);
    VD_REQUIRE(ident_from >= 0 && ident_from <= B, "vd_attention_ident_f16: ident_from = %d is outside [0, %d]", ident_from, B);
    const int64_t HD = (int64_t)H * D;
    VD_REQUIRE(HD % 8 == 0 && ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && sv % 8 == 0 && so % 8 == 0,
               "vd_attention_ident_f16: H * D = %lld, the leading dimensions and the sample strides of v and out must be multiples of 8",
               (long long)HD);
    VD_REQUIRE(ldv >= HD && ldo >= HD, "vd_attention_ident_f16: ldv = %d and ldo = %d must cover the H * D = %lld columns", ldv, ldo,
               (long long)HD);
    VD_REQUIRE(vd_aligned16(v) && vd_aligned16(out), "vd_attention_ident_f16: v and out must be 16-byte aligned (column offsets that are multiples of 8)");
    if (ident_from > 0) {
        const int rc = vd_attention_f16(q, k, v, out, ident_from, H, Nq, Nk, D, ldq, ldk, ldv, ldo, sq, sk, sv, so, scale, 0, stream);
        if (rc < 0) {
            char inner[400];
            snprintf(inner, sizeof(inner), "%s", vd_last_error());
            vd_set_error("vd_attention_ident_f16: %s", inner);
            return rc;
        }
    }
    if (ident_from == B) return VD_OK;
    const int chunks = (int)(HD / 8);
    const size_t work = (size_t)(B - ident_from) * Nq * chunks;
    const f16* v0 = (const f16*)v + (int64_t)ident_from * sv;
    f16* o0 = (f16*)out + (int64_t)ident_from * so;
    hipLaunchKernelGGL(pag_ident_copy_kernel, dim3(grid_for(work, PAG_THREADS, 2048)), dim3(PAG_THREADS), 0, stream, v0, o0, Nq, chunks,
                       ldv, ldo, sv, so, work);
    return vd_check_launch("vd_attention_ident_f16");
}

extern "C" int vd_pag_fold_f16(void* eps, int64_t n, int reps, const float* w, hipStream_t stream) {
    VD_REQUIRE(eps && w, "vd_pag_fold_f16: null pointer");
    VD_REQUIRE(n > 0, "vd_pag_fold_f16: n = %lld must be positive", (long long)n);
    VD_REQUIRE(reps == 2 || reps == 3, "vd_pag_fold_f16: reps = %d, expected 2 ([cond ; perturbed]) or 3 ([uncond ; cond ; perturbed])", reps);
    VD_REQUIRE(((uintptr_t)eps & 1) == 0 && ((uintptr_t)w & 3) == 0, "vd_pag_fold_f16: eps and w must be aligned to their element size");
    if (vd_aligned16(eps) && n % 8 == 0) {
        hipLaunchKernelGGL(pag_fold_kernel<true>, dim3(grid_for((size_t)(n / 8), PAG_THREADS, 2048)), dim3(PAG_THREADS), 0, stream,
                           (f16*)eps, n, reps, w);
    } else {
        hipLaunchKernelGGL(pag_fold_kernel<false>, dim3(grid_for((size_t)n, PAG_THREADS, 2048)), dim3(PAG_THREADS), 0, stream, (f16*)eps,
                           n, reps, w);
    }
    return vd_check_launch("vd_pag_fold_f16");
}
