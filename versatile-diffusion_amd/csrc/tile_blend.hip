// Tiled VAE decode / encode (gfx950): tile_blend fuses the per-tile outputs of the KL-f8 decoder (the raw image, C = 3) or of
// quant_conv (the moments, C = 2 zc) back into one canvas -- the weighted sum over the covering tiles, the normalisation, the
// affine and clamp of the image, and the layout change, in one pass.  Contract (layouts, the order of the sum, the roundings):
// include/vd_hip.h; the tables: lib/model_zoo/windows.py through lib/model_zoo/vae_tiles.py.
// The canvas is an image here (512 x 2048 x 3 per sample and more), so unlike window_merge_kernel one work item owns one canvas
// PIXEL: the coverage test and the wgt / inv_den reads happen once for all C channels, and the C fp16 of a tile pixel, which lie
// together in the channels-last tile, are read together.  Lanes are consecutive along X, so a wave reads runs of consecutive
// tile bytes (64 x 2C) per covering tile and writes one run per channel plane (NCHW, acc) or one packed run (NHWC).
#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

// fp32 -> fp16 as a rounding of its own (unipc.hip's rule): left to the compiler, the conversion would be folded into the
// arithmetic in front of it (v_fma_mixlo_f16), which rounds the exact result once to fp16.  The empty asm keeps the fp32 value.
__device__ __forceinline__ f16 tile_round_f16(float v) {
    asm("" : "+v"(v));
    return (f16)v;
}

// C consecutive fp16 at p, moved V at a time (V divides C; 2 V-byte accesses, the host has checked the alignment)
template <int V> struct TileVec { typedef f16 type __attribute__((ext_vector_type(V))); };

template <int C, int V>
__device__ __forceinline__ void tile_load(const f16* p, float (&v)[C]) {
    if constexpr (V == 1) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = (float)p[c];
    } else {
        typedef typename TileVec<V>::type vec;
#pragma unroll
        for (int g = 0; g < C / V; ++g) {
            const vec x = *reinterpret_cast<const vec*>(p + g * V);
#pragma unroll
            for (int e = 0; e < V; ++e) v[g * V + e] = (float)x[e];
        }
    }
}

template <int C, int V>
__device__ __forceinline__ void tile_store(f16* p, const f16 (&v)[C]) {
    if constexpr (V == 1) {
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = v[c];
    } else {
        typedef typename TileVec<V>::type vec;
#pragma unroll
        for (int g = 0; g < C / V; ++g) {
            vec x;
#pragma unroll
            for (int e = 0; e < V; ++e) x[e] = v[g * V + e];
            *reinterpret_cast<vec*>(p + g * V) = x;
        }
    }
}

// One work item = one canvas pixel (rb, Y, X), all C channels in registers.  The tiles are walked in ascending order -- a gather,
// so the order of the sum is fixed and nothing is atomic.  Whether tile k covers the pixel is decided from the pixel's side --
// i = Y - oy in [0, ph), j = X - ox (+ PW when wrapping and negative) in [0, pw) -- so every tile index is in bounds whatever
// the table holds.  The grid is (runs of 256 columns, rows, samples): X, Y and rb come from the block and thread indices with no
// division, Y and with it the row test are uniform over a block, and the table reads are uniform over the grid (scalar loads);
// wgt and inv_den are small and stay in L2.
template <int C, int V>
__global__ void __launch_bounds__(256) tile_blend_kernel(const f16* tiles, float* acc, f16* out, const float* wgt,
                                                         const float* inv_den, const int32_t* offs, int RB, int PH, int PW, int ph,
                                                         int pw, int slots, int valid, int wrap, int first, int last,
                                                         int out_nhwc, float scale, float shift, int clamp01) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x;
    if (X >= PW) return;
    const size_t plane = (size_t)PH * PW;
    const size_t tpix = (size_t)ph * pw;
    for (int rb = blockIdx.z; rb < RB; rb += gridDim.z) {
        for (int Y = blockIdx.y; Y < PH; Y += gridDim.y) {
            const size_t yx = (size_t)Y * PW + X;
            float* accp = acc ? acc + (size_t)rb * C * plane + yx : nullptr;
            float a[C];
            if (first) {
#pragma unroll
                for (int c = 0; c < C; ++c) a[c] = 0.f;
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) a[c] = accp[c * plane];
            }
            for (int k = 0; k < valid; ++k) {
                const int i = Y - offs[2 * k];
                if (i < 0 || i >= ph) continue;
                int j = X - offs[2 * k + 1];
                if (wrap && j < 0) j += PW;         // 0 <= ox < PW in a wrapped table: one step brings j into [0, PW)
                if (j < 0 || j >= pw) continue;
                const size_t p = (size_t)i * pw + j;
                const float wv = wgt[p];
                float v[C];
                tile_load<C, V>(tiles + (((size_t)rb * slots + k) * tpix + p) * C, v);
#pragma unroll
                for (int c = 0; c < C; ++c) a[c] = fmaf(wv, v[c], a[c]);
            }
            if (!(first && last)) {
#pragma unroll
                for (int c = 0; c < C; ++c) accp[c * plane] = a[c];
            }
            if (last) {
                const float inv = inv_den[yx];
                f16 o[C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float r = a[c] * inv;
                    asm("" : "+v"(r));              // the product is rounded to fp32 before the affine sees it
                    r = fmaf(r, scale, shift);
                    if (clamp01) r = fminf(fmaxf(r, 0.f), 1.f);
                    o[c] = tile_round_f16(r);
                }
                if (out_nhwc) {
                    tile_store<C, V>(out + ((size_t)rb * plane + yx) * C, o);
                } else {
                    f16* op = out + (size_t)rb * C * plane + yx;
#pragma unroll
                    for (int c = 0; c < C; ++c) op[c * plane] = o[c];
                }
            }
        }
    }
}

typedef void (*tile_blend_fn)(const f16*, float*, f16*, const float*, const float*, const int32_t*, int, int, int, int, int, int,
                              int, int, int, int, int, float, float, int);

// the widest access (in fp16 elements, at most 8 = 16 bytes) that divides C
constexpr int tile_vec_of(int C) { return C % 8 == 0 ? 8 : (C % 4 == 0 ? 4 : (C % 2 == 0 ? 2 : 1)); }

template <int C>
tile_blend_fn tile_blend_pick(bool vec) {
    return vec ? tile_blend_kernel<C, tile_vec_of(C)> : tile_blend_kernel<C, 1>;
}

}  // namespace

extern "C" int vd_tile_blend_f16(const void* tiles, float* acc, void* out, const float* wgt, const float* inv_den,
                                 const int32_t* offs, int RB, int C, int PH, int PW, int ph, int pw, int slots, int valid,
                                 int wrap, int first, int last, int out_nhwc, float scale, float shift, int clamp01,
                                 hipStream_t stream) {
    first = first != 0;
    last = last != 0;
    VD_REQUIRE(tiles && wgt && inv_den && offs, "vd_tile_blend_f16: null pointer");
    VD_REQUIRE(acc || (first && last), "vd_tile_blend_f16: acc may be NULL only when first && last");
    VD_REQUIRE(out || !last, "vd_tile_blend_f16: the last launch needs out");
    VD_REQUIRE(RB > 0 && PH > 0 && PW > 0 && ph > 0 && pw > 0 && slots > 0, "vd_tile_blend_f16: sizes must be positive");
    VD_REQUIRE(C >= 1 && C <= 16, "vd_tile_blend_f16: C = %d outside [1, 16]", C);
    VD_REQUIRE(ph <= PH && pw <= PW, "vd_tile_blend_f16: tile %d x %d does not fit the canvas %d x %d", ph, pw, PH, PW);
    VD_REQUIRE(valid >= 1 && valid <= slots, "vd_tile_blend_f16: valid = %d outside [1, %d]", valid, slots);
    // torch slices can start anywhere: the wide accesses only when the tiles and a channels-last out start on their boundary
    // (a pixel then starts on it too, 2 C bytes being a multiple of the access)
    const uintptr_t bytes = 2 * (uintptr_t)tile_vec_of(C);
    const bool vec = ((uintptr_t)tiles % bytes) == 0 && (!(last && out_nhwc) || ((uintptr_t)out % bytes) == 0);
    tile_blend_fn fn = nullptr;
    switch (C) {
#define VD_TILE_CASE(N) case N: fn = tile_blend_pick<N>(vec); break;
        VD_TILE_CASE(1) VD_TILE_CASE(2) VD_TILE_CASE(3) VD_TILE_CASE(4) VD_TILE_CASE(5) VD_TILE_CASE(6) VD_TILE_CASE(7)
        VD_TILE_CASE(8) VD_TILE_CASE(9) VD_TILE_CASE(10) VD_TILE_CASE(11) VD_TILE_CASE(12) VD_TILE_CASE(13) VD_TILE_CASE(14)
        VD_TILE_CASE(15) VD_TILE_CASE(16)
#undef VD_TILE_CASE
    }
    const dim3 grid((PW + 255) / 256, PH < 65535 ? PH : 65535, RB < 65535 ? RB : 65535);
    hipLaunchKernelGGL(fn, grid, dim3(256), 0, stream, (const f16*)tiles, acc, (f16*)out, wgt, inv_den, offs, RB, PH, PW, ph, pw,
                       slots, valid, wrap != 0, first, last, out_nhwc != 0, scale, shift, clamp01 != 0);
    return vd_check_launch("vd_tile_blend_f16");
}
