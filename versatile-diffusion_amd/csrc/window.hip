// Windowed (MultiDiffusion) sampling, the kernels around the UNet forward of a step (gfx950): window_gather cuts the canvas
// latent into the batch of windows the UNet sees, window_merge fuses the windows' predictions back into one canvas-shaped
// prediction, window_merge_masked does the same for one region of a regional-prompt call (a mask per launch).  Contract (layouts, the order of the sum, the roundings): include/vd_hip.h; the tables: lib/model_zoo/windows.py.
// The canvas is small (4 x 64 x 256 elements per sample), so both kernels are the plain form: one work item per output piece,
// consecutive lanes on consecutive addresses, no shared memory, no atomics.
#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

// fp32 -> fp16 as a rounding of its own (unipc.hip's rule): left to the compiler, the conversion would be folded into the
// multiply in front of it (v_fma_mixlo_f16), which rounds the exact product once to fp16.  The empty asm keeps the fp32 value.
__device__ __forceinline__ f16 window_round_f16(float v) {
    asm("" : "+v"(v));
    return (f16)v;
}

// A window's offset as the gather uses it: offsets are not validated by the entry points, so a row of the table
// that lies outside the canvas is brought inside here -- a bad table then reads the wrong pixels, never out of bounds.
__device__ __forceinline__ bool window_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
__device__ __forceinline__ int window_clamp(int o, int hi) { return o < 0 ? 0 : (o > hi ? hi : o); }
__device__ __forceinline__ int window_mod(int v, int W) {
    const int r = v % W;
    return r < 0 ? r + W : r;
}

// One work item = up to 8 consecutive elements of one window row: (b, k, c, i, segment).  Consecutive lanes take consecutive
// segments of a row, then the next row, so a wave reads and writes runs of consecutive addresses.  A segment moves as one
// 16-byte access when it is whole, does not cross the wrap seam and both of its addresses are 16-byte aligned; else as 2-byte
// accesses of the same elements.  Either way the copy is bit-exact.
__global__ void window_gather_kernel(const f16* x, f16* win, const int32_t* offs, int C, int H, int W, int h, int w,
                                     int slots, int wrap, size_t work) {
    const int segs = (w + 7) / 8;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < work; t += stride) {
        size_t r = t;
        const int seg = (int)(r % segs); r /= segs;
        const int i = (int)(r % h); r /= h;
        const int c = (int)(r % C); r /= C;
        const int k = (int)(r % slots);
        const size_t b = r / slots;
        const int oy = window_clamp(offs[2 * k], H - h);
        const int ox = wrap ? window_mod(offs[2 * k + 1], W) : window_clamp(offs[2 * k + 1], W - w);
        const int j0 = seg * 8;
        const int nj = w - j0 < 8 ? w - j0 : 8;
        const f16* src_row = x + ((b * C + c) * H + (size_t)(oy + i)) * W;
        f16* dst = win + ((((b * slots + k) * C + c) * h + (size_t)i) * w + j0);
        int col = ox + j0;
        if (wrap && col >= W) col -= W;
        const f16* src = src_row + col;
        if (nj == 8 && col + 8 <= W && window_aligned16(src) && window_aligned16(dst)) {
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
        } else {
            for (int j = 0; j < nj; ++j) {
                int cj = col + j;
                if (cj >= W) cj -= W;               // only with wrap: without it ox + w <= W
                dst[j] = src_row[cj];
            }
        }
    }
}

// One thread owns one canvas element (rb, c, Y, X) and walks the windows in ascending order: a gather, so the order of the
// sum is fixed and nothing is atomic.  Whether window k covers the pixel is decided from the pixel's side -- i = Y - oy in
// [0, h), j = X - ox (mod W when wrapping) in [0, w) -- so every eps_win index is in bounds whatever the table holds.  The
// table reads are uniform over the grid (scalar loads).  With w <= W a wrapped window covers a column at most once.
__global__ void window_merge_kernel(const f16* eps_win, float* acc, f16* eps, const float* wgt, const float* inv_den,
                                    const int32_t* offs, int C, int H, int W, int h, int w, int slots, int valid, int wrap,
                                    int first, int last, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t hw = (size_t)h * w;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        size_t r = t;
        const int X = (int)(r % W); r /= W;
        const int Y = (int)(r % H); r /= H;
        const int c = (int)(r % C);
        const size_t rb = r / C;
        float a = first ? 0.f : acc[t];
        for (int k = 0; k < valid; ++k) {
            const int i = Y - offs[2 * k];
            if (i < 0 || i >= h) continue;
            int j = X - offs[2 * k + 1];
            if (wrap) j = window_mod(j, W);
            if (j < 0 || j >= w) continue;
            const size_t p = (size_t)i * w + j;
            a = fmaf(wgt[p], (float)eps_win[((rb * slots + k) * C + c) * hw + p], a);
        }
        if (!(first && last)) acc[t] = a;
        if (last) eps[t] = window_round_f16(a * inv_den[(size_t)Y * W + X]);
    }
}

// window_merge_kernel for one region of a regional-prompt call: the same thread layout, coverage test and order, with the
// region's mask value of the pixel multiplied into the weight -- wm = wgt * mask as an fp32 product of its own, then the same
// fmaf.  A pixel the region does not own (mask 0) skips the windows altogether, so whatever the UNet predicted there (a NaN
// included) never meets the sum.  first / last span all (region, chunk) launches of a step.
__global__ void window_merge_masked_kernel(const f16* eps_win, float* acc, f16* eps, const float* wgt, const float* mask,
                                           const float* inv_den, const int32_t* offs, int C, int H, int W, int h, int w,
                                           int slots, int valid, int wrap, int first, int last, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t hw = (size_t)h * w;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        size_t r = t;
        const int X = (int)(r % W); r /= W;
        const int Y = (int)(r % H); r /= H;
        const int c = (int)(r % C);
        const size_t rb = r / C;
        float a = first ? 0.f : acc[t];
        const float mv = mask[(size_t)Y * W + X];
        if (mv != 0.f) {
            for (int k = 0; k < valid; ++k) {
                const int i = Y - offs[2 * k];
                if (i < 0 || i >= h) continue;
                int j = X - offs[2 * k + 1];
                if (wrap) j = window_mod(j, W);
                if (j < 0 || j >= w) continue;
                const size_t p = (size_t)i * w + j;
                const float wm = wgt[p] * mv;
                a = fmaf(wm, (float)eps_win[((rb * slots + k) * C + c) * hw + p], a);
            }
        }
        if (!(first && last)) acc[t] = a;
        if (last) eps[t] = window_round_f16(a * inv_den[(size_t)Y * W + X]);
    }
}

}  // namespace

extern "C" int vd_window_gather_f16(const void* x, void* win, const int32_t* offs, int B, int C, int H, int W, int h, int w,
                                    int slots, int wrap, hipStream_t stream) {
    VD_REQUIRE(x && win && offs, "vd_window_gather_f16: null pointer");
    VD_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0 && slots > 0, "vd_window_gather_f16: sizes must be positive");
    VD_REQUIRE(h <= H && w <= W, "vd_window_gather_f16: window %d x %d does not fit the canvas %d x %d", h, w, H, W);
    const size_t work = (size_t)B * slots * C * h * ((w + 7) / 8);
    hipLaunchKernelGGL(window_gather_kernel, dim3(grid_for(work)), dim3(256), 0, stream, (const f16*)x, (f16*)win, offs, C, H,
                       W, h, w, slots, wrap != 0, work);
    return vd_check_launch("vd_window_gather_f16");
}

extern "C" int vd_window_merge_f16(const void* eps_win, float* acc, void* eps, const float* wgt, const float* inv_den,
                                   const int32_t* offs, int RB, int C, int H, int W, int h, int w, int slots, int valid,
                                   int wrap, int first, int last, hipStream_t stream) {
    first = first != 0;
    last = last != 0;
    VD_REQUIRE(eps_win && wgt && inv_den && offs, "vd_window_merge_f16: null pointer");
    VD_REQUIRE(acc || (first && last), "vd_window_merge_f16: acc may be NULL only when first && last");
    VD_REQUIRE(eps || !last, "vd_window_merge_f16: the last launch needs eps");
    VD_REQUIRE(RB > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0 && slots > 0, "vd_window_merge_f16: sizes must be positive");
    VD_REQUIRE(h <= H && w <= W, "vd_window_merge_f16: window %d x %d does not fit the canvas %d x %d", h, w, H, W);
    VD_REQUIRE(valid >= 1 && valid <= slots, "vd_window_merge_f16: valid = %d outside [1, %d]", valid, slots);
    const size_t n = (size_t)RB * C * H * W;
    hipLaunchKernelGGL(window_merge_kernel, dim3(grid_for(n)), dim3(256), 0, stream, (const f16*)eps_win, acc, (f16*)eps, wgt,
                       inv_den, offs, C, H, W, h, w, slots, valid, wrap != 0, first, last, n);
    return vd_check_launch("vd_window_merge_f16");
}

extern "C" int vd_window_merge_masked_f16(const void* eps_win, float* acc, void* eps, const float* wgt, const float* mask,
                                          const float* inv_den, const int32_t* offs, int RB, int C, int H, int W, int h, int w,
                                          int slots, int valid, int wrap, int first, int last, hipStream_t stream) {
    first = first != 0;
    last = last != 0;
    VD_REQUIRE(eps_win && wgt && mask && inv_den && offs, "vd_window_merge_masked_f16: null pointer");
    VD_REQUIRE(acc || (first && last), "vd_window_merge_masked_f16: acc may be NULL only when first && last");
    VD_REQUIRE(eps || !last, "vd_window_merge_masked_f16: the last launch needs eps");
    VD_REQUIRE(RB > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0 && slots > 0,
               "vd_window_merge_masked_f16: sizes must be positive");
    VD_REQUIRE(h <= H && w <= W, "vd_window_merge_masked_f16: window %d x %d does not fit the canvas %d x %d", h, w, H, W);
    VD_REQUIRE(valid >= 1 && valid <= slots, "vd_window_merge_masked_f16: valid = %d outside [1, %d]", valid, slots);
    const size_t n = (size_t)RB * C * H * W;
    hipLaunchKernelGGL(window_merge_masked_kernel, dim3(grid_for(n)), dim3(256), 0, stream, (const f16*)eps_win, acc, (f16*)eps,
                       wgt, mask, inv_den, offs, C, H, W, h, w, slots, valid, wrap != 0, first, last, n);
    return vd_check_launch("vd_window_merge_masked_f16");
}
