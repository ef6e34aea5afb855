// FreeU (Si et al., CVPR 2024) at a skip concatenation of the UNet's decoder (gfx950): the backbone tensor h gets the first half of
// its channels scaled, the skip tensor gets the lowest frequencies of every H x W plane damped.  Contract (the seven sums, the
// tables, the roundings): include/vd_hip.h.  One launch does both: the first B * C1 / 8 blocks filter the skip, the blocks behind
// them scale and copy h.
//
// Skip blocks.  A block owns 8 consecutive channels (one 16-byte access per pixel) of one sample over all H * W pixels:
// B = 1 at C1 = 640 is 80 blocks, the guided pair 160, width 1280 twice that -- every plane of these levels (8 x 8 to 64 x 64, at
// most 2.6 MB per sample) stays in L2, so the second read of x costs no HBM traffic.  Phase 1: thread t of the block's 256 takes
// pixels t, t + 256, .. in ascending order and keeps the 7 sums of its 8 channels in 56 registers; a wave sums them by the xor
// butterfly (32, 16, .. 1), wave 0 .. 3 are added in that order through LDS.  The order depends on H * W alone: nothing is atomic,
// no block sees another sample.  (Measured, profiles/HISTORY.md: blocks of 512 / 1024 threads for planes above 1024 / 2048 pixels
// took 90 us where 256 threads take 75 us on the 64 x 64 load of the bench geometry, so the block does not grow with the plane.)
// Phase 2 reads x again and stores y.  The trig tables come from the host (no trig here); their reads are the same address for
// the 8 channels of a thread and consecutive addresses over the lanes.
#include "vd_common.h"
#include "../../include/vd_hip.h"

namespace {

constexpr int FREEU_THREADS = 256;
constexpr int FREEU_SUMS = 7 * 8;      // S0, Ay, By, Ax, Bx, Axy, Bxy of 8 channels

// fp32 -> fp16 as a rounding of its own (window.hip's rule): left to the compiler, the conversion is folded into the multiply or
// fma in front of it (v_fma_mixlo_f16), which rounds the exact result once to fp16.  The empty asm keeps the fp32 value.
__device__ __forceinline__ f16 freeu_round_f16(float v) {
    asm("" : "+v"(v));
    return (f16)v;
}

struct FreeuTables {
    const float *cy, *sy, *cx, *sx, *cxy, *sxy;
};

__global__ __launch_bounds__(FREEU_THREADS) void freeu_kernel(const f16* h, const f16* skip, f16* h_out, f16* skip_out, FreeuTables tab,
                                                             int HW, int W, int C0, int C1, unsigned nskip, size_t back_work, float b,
                                                             float g) {
    __shared__ float part[FREEU_THREADS / 64][FREEU_SUMS];
    __shared__ float total[FREEU_SUMS];
    const int tid = threadIdx.x;
    constexpr int T = FREEU_THREADS;
    if (blockIdx.x >= nskip) {
        // backbone: one work item = 8 channels of one pixel; channel c < C0 / 2 is scaled, the others are copied
        const int chunks = C0 / 8, half = C0 / 2;
        const size_t stride = (size_t)(gridDim.x - nskip) * T;
        for (size_t t = (size_t)(blockIdx.x - nskip) * T + tid; t < back_work; t += stride) {
            const int c0 = (int)(t % chunks) * 8;
            U4H8 v;
            v.u = *reinterpret_cast<const uint4*>(h + t * 8);
            if (c0 < half) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (c0 + j < half) v.e[j] = freeu_round_f16((float)v.e[j] * b);
            }
            *reinterpret_cast<uint4*>(h_out + t * 8) = v.u;
        }
        return;
    }
    const int chunks = C1 / 8;
    const size_t sample = blockIdx.x / chunks;
    const f16* x = skip + sample * HW * C1 + (size_t)(blockIdx.x % chunks) * 8;
    f16* y = skip_out + sample * HW * C1 + (size_t)(blockIdx.x % chunks) * 8;

    float acc[FREEU_SUMS];
#pragma unroll
    for (int k = 0; k < FREEU_SUMS; ++k) acc[k] = 0.f;
    for (int i = tid; i < HW; i += T) {
        const int p = i / W, q = i - p * W;
        const float t1 = tab.cy[p], t2 = tab.sy[p], t3 = tab.cx[q], t4 = tab.sx[q], t5 = tab.cxy[i], t6 = tab.sxy[i];
        U4H8 v;
        v.u = *reinterpret_cast<const uint4*>(x + (size_t)i * C1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float xv = (float)v.e[j];
            acc[j] += xv;
            acc[8 + j] = fmaf(xv, t1, acc[8 + j]);
            acc[16 + j] = fmaf(xv, t2, acc[16 + j]);
            acc[24 + j] = fmaf(xv, t3, acc[24 + j]);
            acc[32 + j] = fmaf(xv, t4, acc[32 + j]);
            acc[40 + j] = fmaf(xv, t5, acc[40 + j]);
            acc[48 + j] = fmaf(xv, t6, acc[48 + j]);
        }
    }
#pragma unroll
    for (int k = 0; k < FREEU_SUMS; ++k) acc[k] = wave_sum(acc[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < FREEU_SUMS; ++k) part[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid < FREEU_SUMS) {
        float s = part[0][tid];
#pragma unroll
        for (int w = 1; w < T / 64; ++w) s += part[w][tid];
        total[tid] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FREEU_SUMS; ++k) acc[k] = total[k];

    for (int i = tid; i < HW; i += T) {
        const int p = i / W, q = i - p * W;
        const float t1 = tab.cy[p], t2 = tab.sy[p], t3 = tab.cx[q], t4 = tab.sx[q], t5 = tab.cxy[i], t6 = tab.sxy[i];
        U4H8 v;
        v.u = *reinterpret_cast<const uint4*>(x + (size_t)i * C1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = acc[j];
            t = fmaf(acc[8 + j], t1, t);
            t = fmaf(acc[16 + j], t2, t);
            t = fmaf(acc[24 + j], t3, t);
            t = fmaf(acc[32 + j], t4, t);
            t = fmaf(acc[40 + j], t5, t);
            t = fmaf(acc[48 + j], t6, t);
            v.e[j] = freeu_round_f16(fmaf(g, t, (float)v.e[j]));
        }
        *reinterpret_cast<uint4*>(y + (size_t)i * C1) = v.u;
    }
}

}  // namespace

extern "C" int vd_freeu_f16(const void* h, const void* skip, void* h_out, void* skip_out, const float* cy, const float* sy,
                            const float* cx, const float* sx, const float* cxy, const float* sxy, int B, int H, int W, int C0,
                            int C1, float b, float s, hipStream_t stream) {
    VD_REQUIRE(h && skip && h_out && skip_out && cy && sy && cx && sx && cxy && sxy, "vd_freeu_f16: null pointer");
    VD_REQUIRE(B > 0 && C0 > 0 && C1 > 0, "vd_freeu_f16: sizes must be positive");
    VD_REQUIRE(H >= 2 && W >= 2, "vd_freeu_f16: the plane is %d x %d, H and W must be at least 2", H, W);
    VD_REQUIRE(C0 % 8 == 0 && C1 % 8 == 0, "vd_freeu_f16: C0 = %d and C1 = %d must be multiples of 8", C0, C1);
    VD_REQUIRE((int64_t)H * W <= (1 << 24), "vd_freeu_f16: the plane %d x %d has more than 2^24 pixels", H, W);
    VD_REQUIRE(h != h_out && skip != skip_out, "vd_freeu_f16: the outputs must not alias the inputs");
    VD_REQUIRE(vd_aligned16(h) && vd_aligned16(skip) && vd_aligned16(h_out) && vd_aligned16(skip_out),
               "vd_freeu_f16: the tensors must be 16-byte aligned");
    VD_REQUIRE(b == b && s == s && b - b == 0.f && s - s == 0.f, "vd_freeu_f16: b and s must be finite");
    const int HW = H * W;
    const size_t nskip = (size_t)B * (C1 / 8);
    const size_t back_work = (size_t)B * HW * (C0 / 8);
    const int nback = grid_for(back_work, FREEU_THREADS, 2048);
    VD_REQUIRE(nskip + nback < (1u << 31), "vd_freeu_f16: B * C1 / 8 = %zu blocks exceed the grid", nskip);
    const float g = (float)(((double)s - 1.0) / (double)HW);
    const FreeuTables tab = {cy, sy, cx, sx, cxy, sxy};
    hipLaunchKernelGGL(freeu_kernel, dim3((unsigned)(nskip + nback)), dim3(FREEU_THREADS), 0, stream, (const f16*)h, (const f16*)skip,
                       (f16*)h_out, (f16*)skip_out, tab, HW, W, C0, C1, (unsigned)nskip, back_work, b, g);
    return vd_check_launch("vd_freeu_f16");
}
