// HyperTile (tfernd, "HyperTile: Tiled-optimizations for Stable-Diffusion", 2023) on gfx950: the two launches a tiled
// self-attention adds.  Contracts: include/vd_hip.h.
//
// Both kernels are one fixed permutation of 16-byte row chunks.  A thread owns one chunk; the chunk index runs fastest, so the
// consecutive lanes of a wave take consecutive 16-byte chunks of ONE row (and go on into the next row of the same tile, which in
// the tiled tensor is adjacent): every wave reads and writes whole cache lines on both sides.  The row arithmetic is 32-bit (the
// entries refuse a problem of 2^32 chunks or more), the byte offsets are 64-bit.  No LDS: nothing is reused.
#include <stdio.h>

#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

constexpr int HT_THREADS = 256;

struct HtGrid {
    int N, W, tw, ntx, tile_rows;   // tokens per sample, grid width, tile width, tiles per grid row, th * tw
};

// row g of the tiled tensor [B nty ntx, th tw, *] -> (sample b, token n of its H x W grid)
__device__ __forceinline__ void ht_source(const HtGrid& s, uint32_t g, uint32_t* b, uint32_t* n) {
    const uint32_t bb = g / (uint32_t)s.N, rem = g - bb * (uint32_t)s.N;
    const uint32_t tile = rem / (uint32_t)s.tile_rows, within = rem - tile * (uint32_t)s.tile_rows;
    const uint32_t ty = tile / (uint32_t)s.ntx, tx = tile - ty * (uint32_t)s.ntx;
    const uint32_t i = within / (uint32_t)s.tw, j = within - i * (uint32_t)s.tw;
    const uint32_t th = (uint32_t)s.tile_rows / (uint32_t)s.tw;
    *b = bb;
    *n = (ty * th + i) * (uint32_t)s.W + tx * (uint32_t)s.tw + j;
}

// TILE: t[g] = x[b, n] (x strided, t contiguous);  else: x[b, n] = t[g]
template <bool TILE>
__global__ __launch_bounds__(HT_THREADS) void hypertile_rows_kernel(const f16* __restrict__ src, f16* __restrict__ dst, int ldx, int64_t sx,
                                                                    int chunks, HtGrid s, uint32_t work) {
    const uint32_t stride = gridDim.x * HT_THREADS;
    for (uint32_t t = blockIdx.x * HT_THREADS + threadIdx.x; t < work; t += stride) {
        // (work < 2^32, but t + stride may wrap: the check below ends the loop then)
        const uint32_t g = t / (uint32_t)chunks, c = t - g * (uint32_t)chunks;
        uint32_t b, n;
        ht_source(s, g, &b, &n);
        const int64_t tiled = ((int64_t)g * chunks + c) * 8;
        const int64_t grid = (int64_t)b * sx + (int64_t)n * ldx + (int64_t)c * 8;
        if (TILE)
            *reinterpret_cast<uint4*>(dst + tiled) = *reinterpret_cast<const uint4*>(src + grid);
        else
            *reinterpret_cast<uint4*>(dst + grid) = *reinterpret_cast<const uint4*>(src + tiled);
        if (t + stride < t) break;
    }
}

// the checks the two entries share; what: the entry's name.  (x, ldx, sx): the [B, H W, cols] side; t: the contiguous tiled side
int ht_ok(const char* what, const void* x, int ldx, int64_t sx, const void* t, int cols, int B, int H, int W, int th, int tw) {
    VD_REQUIRE(x && t, "%s: null pointer", what);
    VD_REQUIRE(B > 0 && H > 0 && W > 0 && th > 0 && tw > 0 && cols > 0, "%s: non-positive size B=%d H=%d W=%d th=%d tw=%d cols=%d", what,
               B, H, W, th, tw, cols);
    VD_REQUIRE(cols % 8 == 0, "%s: cols = %d must be a multiple of 8", what, cols);
    VD_REQUIRE(H % th == 0 && W % tw == 0, "%s: the tile %d x %d does not divide the token grid %d x %d", what, th, tw, H, W);
    VD_REQUIRE(ldx >= cols, "%s: the leading dimension %d is below cols = %d", what, ldx, cols);
    VD_REQUIRE(vd_aligned16(x) && vd_aligned16(t) && ldx % 8 == 0 && sx % 8 == 0,
               "%s: the tensors must be 16-byte aligned and the leading dimension %d and the sample stride %lld multiples of 8", what, ldx,
               (long long)sx);
    // the strided side must hold its rows without overlap: a sample's last row ends inside the sample stride (B > 1)
    VD_REQUIRE(B == 1 || sx >= ((int64_t)H * W - 1) * ldx + cols, "%s: the sample stride %lld is below the %d rows of a sample", what,
               (long long)sx, H * W);
    VD_REQUIRE((int64_t)B * H * W * (cols / 8) < ((int64_t)1 << 32), "%s: B H W cols / 8 = %lld chunks, at most 2^32 - 1", what,
               (long long)B * H * W * (cols / 8));
    return VD_OK;
}

template <bool TILE>
int ht_launch(const char* what, const void* src, void* dst, int ldx, int64_t sx, int cols, int B, int H, int W, int th, int tw,
              hipStream_t stream) {
    const int chunks = cols / 8;
    const HtGrid s = {H * W, W, tw, W / tw, th * tw};
    const size_t work = (size_t)B * H * W * chunks;
    hipLaunchKernelGGL(hypertile_rows_kernel<TILE>, dim3(grid_for(work, HT_THREADS, 8192)), dim3(HT_THREADS), 0, stream, (const f16*)src,
                       (f16*)dst, ldx, sx, chunks, s, (uint32_t)work);
    return vd_check_launch(what);
}

}  // namespace

extern "C" int vd_tile_tokens_f16(const void* x, int ldx, int64_t sx, int cols, int B, int H, int W, int th, int tw, void* out,
                                  hipStream_t stream) {
    if (int rc = ht_ok("vd_tile_tokens_f16", x, ldx, sx, out, cols, B, H, W, th, tw)) return rc;
    return ht_launch<true>("vd_tile_tokens_f16", x, out, ldx, sx, cols, B, H, W, th, tw, stream);
}

extern "C" int vd_untile_tokens_f16(const void* a, int cols, int B, int H, int W, int th, int tw, void* out, int ldo, int64_t so,
                                    hipStream_t stream) {
    if (int rc = ht_ok("vd_untile_tokens_f16", out, ldo, so, a, cols, B, H, W, th, tw)) return rc;
    return ht_launch<false>("vd_untile_tokens_f16", a, out, ldo, so, cols, B, H, W, th, tw, stream);
}
