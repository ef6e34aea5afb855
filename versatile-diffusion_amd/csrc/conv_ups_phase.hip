// vd_conv3x3_ups_phase_f16: the 3x3 convolution behind a nearest-2x upsample (Upsample.conv of the UNet and of the VAE decoder,
// lib/model_zoo/openaimodel.py:89-117, autokl_modules.py:42-56) as four 2x2 PHASE convolutions of the low-resolution image --
// the TAPS = 4 instances of conv3x3_halo_kernel (conv_halo_kernel.h), their geometry and their launch planner.  In its own
// translation unit: the 3x3 instances of conv_halo.hip are compiled exactly as before.
//
//   out[2i + a][2j + b][n] = sum_{p, q in {0, 1}} sum_c Wph[a][b][n][p][q][c] * x[i + a - 1 + p][j + b - 1 + q][c]
//   Wph[a][b][n][p][q][c]  = sum_{ky in R(a, p)} sum_{kx in R(b, q)} w[n][ky][kx][c],   R(0,0) = {0}, R(0,1) = {1,2}, R(1,0) = {0,1}, R(1,1) = {2}
//
// The nine taps of the upsampled form read every source pixel up to four times with different weights; summing those weights once
// (fp32 sums of the fp16 weights, one rounding to fp16: vd_hip/pack.py) leaves 4 C instead of 9 C multiplies per output.  A source
// index outside the image reads zero, which is the zero padding of the upsampled image.  Exact algebra with one added weight rounding.
#include "conv_halo_kernel.h"

// gemm.hip
int vd_gemm_normalise(const VdGemmDesc* desc, void* gemm_args_out);
int vd_gemm_launch_reduce(const void* gemm_args, int nsplit, hipStream_t stream);

namespace {

// ---- The built instances: the planner's tile and the VAE's tile of conv_halo.hip with four taps. ---------------------------
//   X(variant, BM, BN, WM, WN, NT)
#define VD_PHASE_VARIANTS(X)        \
    X(0, 256, 160, 32, 160, 512)    \
    X(1, 256, 128, 64,  64, 512)

struct PhaseVariant { int bm, bn; const char* name; };
constexpr PhaseVariant kPhase[] = {
#define X(v, BM, BN, WM, WN, NT) {BM, BN, "conv3x3_halo_kernel<" #BM "," #BN "," #WM "," #WN "," #NT ",2,phase4>"},
    VD_PHASE_VARIANTS(X)
#undef X
};
constexpr int kNumPhase = (int)(sizeof(kPhase) / sizeof(kPhase[0]));

inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// Patch geometry on the LOW-RESOLUTION grid for BM pixels of one phase per block; false when the convolution does not fit.
// `a` is the normalised descriptor of the upsampled 3x3 form (ups = 1, K = 9 C); c.g describes what the kernel reads.
bool phase_geometry(const GemmArgs& a, int BM, const void* w_phase, ConvHaloArgs& c) {
    const VdGemmDesc& d = a.d;
    if (d.ksize != 3 || d.stride != 1 || d.pad != 1 || d.ups != 1 || d.batch != 1) return false;
    if (d.flags & (VD_EPI_LNFOLD | VD_EPI_OUT_F32 | VD_EPI_BIAS_ALONG_M)) return false;
    if (d.act == VD_ACT_GEGLU) return false;
    if (d.a1 != nullptr || d.c1 != 0 || d.skip_a0 != nullptr || d.skip_w != nullptr) return false;   // one source
    if (d.c0 % 64 != 0 || d.N % 8 != 0) return false;
    const int Hl = d.Hin, Wl = d.Win;
    if (d.Hout != 2 * Hl || d.Wout != 2 * Wl) return false;
    const long npix = (long)Hl * Wl;
    if (d.M % (4 * npix) != 0) return false;
    const long nimg = d.M / (4 * npix);
    if (nimg * npix >= (1l << 28)) return false;   // packed (pixel << 3 | slot) source indices
    const int tw = (Wl % 32 == 0) ? 32 : (Wl % 16 == 0) ? 16 : (Wl % 8 == 0) ? 8 : 0;
    if (tw == 0) return false;
    const int th = BM / tw;
    int ngrp, rg;
    if (Hl % th == 0) {
        ngrp = 1;
        rg = th;
    } else if (th % Hl == 0 && tw == Wl && is_pow2(Hl) && nimg % (th / Hl) == 0) {
        ngrp = th / Hl;   // whole small images per patch
        rg = Hl;
    } else {
        return false;
    }
    const size_t wb = (size_t)4 * d.N * 4 * d.c0 * 2;
    if (wb >= (1ull << 31)) return false;
    c.g = a;
    c.g.d.ups = 0;            // the kernel gathers on the low-resolution grid itself
    c.g.d.w = w_phase;        // [4 phases][N][2x2 taps][C]
    c.g.d.ldw = 4 * d.c0;
    c.g.w_bytes = (unsigned)wb;
    c.tw = tw;
    c.ltw = ilog2(tw);
    c.rg = rg;
    c.ngrp = ngrp;
    c.lgsz = ilog2(tw * rg);
    c.pitch = tw + 1;
    c.gpx = (rg + 1) * c.pitch;
    c.hpx = ngrp * c.gpx;
    if (c.hpx > BM * 100 / 64 + 16) return false;
    c.mg_pitch = (1 << 20) / c.pitch + 1;
    c.mg_gpx = (1 << 20) / c.gpx + 1;
    c.tiles_x = Wl / tw;
    c.tiles_y = ngrp == 1 ? Hl / rg : 1;
    c.nchunks = d.c0 / 64;
    c.chunks_per_split = c.nchunks;
    c.Hv = Hl;
    c.Wv = Wl;
    c.halo_bytes = ((c.hpx + 7) / 8) * 1024;
    c.g.tiles_m = 4 * (int)(nimg * npix / BM);   // [phase][low-resolution patch]
    c.abl = 0;
    c.nskip = 0;
    c.skip_cps = 0;
    c.s0_bytes = c.s1_bytes = c.sw_bytes = 0;
    return true;
}

struct PhasePlan { int variant, nsplit, stat_rows; };

// Whether (and how) the normalised upsampled 3x3 problem `a` runs in the phase form.  can_split: a workspace will be there.
bool phase_plan(const GemmArgs& a, const void* w_phase, bool can_split, ConvHaloArgs& c, PhasePlan& pl) {
    const VdGemmDesc& d = a.d;
    int v;
    if (d.N % 160 == 0) v = 0;         // as vd_conv_halo_plan: the planner's tile for every UNet width
    else if (d.N % 128 == 0) v = 1;    // the VAE's 128 / 256 / 512
    else return false;
    const PhaseVariant& pv = kPhase[v];
    if (!phase_geometry(a, pv.bm, w_phase, c)) return false;
    c.g.tiles_n = (d.N + pv.bn - 1) / pv.bn;
    if (2 * c.halo_bytes + 3 * pv.bn * 128 > 160 * 1024) return false;
    // (no lower bound on the tiles as in vd_conv_halo_plan: the alternative for a small grid is the same convolution with 9 / 4 of
    // the work, and the split below fills the chip)
    const long tiles = (long)c.g.tiles_m * c.g.tiles_n;
    // split over channel chunks until one round of blocks covers the chip; unit = one tap of one block (vd_conv_halo_plan's model)
    int ns = 1;
    if (d.split_k > 0) {
        ns = d.split_k;
    } else if (can_split) {
        float best = 1e30f;
        for (int s = 1; s <= c.nchunks && s <= VD_MAX_SPLIT_K / 2; ++s) {
            const int cps = (c.nchunks + s - 1) / s;
            if ((c.nchunks + cps - 1) / cps != s) continue;   // same work per block as a smaller factor
            const long rounds = (tiles * s + 255) / 256;
            const float t = (float)rounds * (cps * 4 + 8) + (s > 1 ? 6.f + 2.f * s : 0.f);
            if (t < best) { best = t; ns = s; }
        }
    }
    if (ns > c.nchunks) ns = c.nchunks;
    if (ns > VD_MAX_SPLIT_K) return false;
    if (ns > 1 && !can_split) ns = 1;
    c.chunks_per_split = (c.nchunks + ns - 1) / ns;
    ns = (c.nchunks + c.chunks_per_split - 1) / c.chunks_per_split;
    // rows per statistics partial (VdGemmDesc.out_stats): a block's BM pixels of one phase (or one phase of a whole small image)
    // when the epilogue runs in the kernel, 64 rows from splitk_reduce_stats_kernel when the chunks are split
    int sr = 0;
    const int HW = d.stat_img_rows;
    if (d.N % 8 == 0 && d.ldc % 8 == 0 && !((d.flags & VD_EPI_RESIDUAL) && d.ldr % 8 != 0) && HW > 0 && d.M % HW == 0) {
        if (ns <= 1) sr = HW != 4 * c.Hv * c.Wv ? 0 : (c.ngrp == 1 ? pv.bm : c.rg * c.tw);
        else sr = HW % 64 == 0 ? 64 : 0;
    }
    pl.variant = v;
    pl.nsplit = ns;
    pl.stat_rows = sr;
    return true;
}

int plan_desc(const VdGemmDesc* dp, const void* w_phase, GemmArgs& a, ConvHaloArgs& c, PhasePlan& pl, bool& ok) {
    VdGemmDesc tmp = *dp;
    tmp.out_stats = nullptr;   // (validated by the caller of this function, not by the planner of the other kernels)
    tmp.stat_sums = nullptr;
    tmp.split_k = 0;           // (the split asked for is this launcher's: the other planner must not demand a workspace for it)
    const int rc = vd_gemm_normalise(&tmp, &a);
    if (rc != VD_OK) return rc;
    a.d.split_k = dp->split_k;
    a.d.out_stats = dp->out_stats;
    a.d.stat_sums = dp->stat_sums;
    a.d.sync = nullptr;   // slabs + the reduce kernel
    ok = phase_plan(a, w_phase, true, c, pl);
    return VD_OK;
}

}  // namespace

extern "C" int vd_conv3x3_ups_phase_supported(const VdGemmDesc* dp) {
    if (dp == nullptr) return 0;
    GemmArgs a;
    ConvHaloArgs c;
    PhasePlan pl;
    bool ok = false;
    if (plan_desc(dp, nullptr, a, c, pl, ok) != VD_OK) return 0;
    return ok ? 1 : 0;
}

extern "C" int vd_conv3x3_ups_phase_plan(const VdGemmDesc* dp, int* variant, int* nsplit, int* stat_rows) {
    VD_REQUIRE(dp != nullptr, "vd_conv3x3_ups_phase_plan: null descriptor");
    GemmArgs a;
    ConvHaloArgs c;
    PhasePlan pl;
    bool ok = false;
    if (const int rc = plan_desc(dp, nullptr, a, c, pl, ok)) return rc;
    VD_REQUIRE(ok, "vd_conv3x3_ups_phase_plan: the geometry does not fit (vd_conv3x3_ups_phase_supported)");
    if (variant) *variant = pl.variant;
    if (nsplit) *nsplit = pl.nsplit;
    if (stat_rows) *stat_rows = pl.stat_rows;
    return VD_OK;
}

extern "C" const char* vd_conv3x3_ups_phase_name(int variant) {
    return (variant >= 0 && variant < kNumPhase) ? kPhase[variant].name : nullptr;
}

extern "C" int vd_conv3x3_ups_phase_f16(const VdGemmDesc* dp, const void* w_phase, hipStream_t stream) {
    VD_REQUIRE(dp != nullptr && w_phase != nullptr, "vd_conv3x3_ups_phase_f16: null argument");
    VD_REQUIRE(((size_t)w_phase & 15) == 0, "vd_conv3x3_ups_phase_f16: w_phase must be 16-byte aligned");
    GemmArgs a;
    ConvHaloArgs c;
    PhasePlan pl;
    bool ok = false;
    if (const int rc = plan_desc(dp, w_phase, a, c, pl, ok)) return rc;
    VD_REQUIRE(ok, "vd_conv3x3_ups_phase_f16: the geometry does not fit (vd_conv3x3_ups_phase_supported)");
    const VdGemmDesc& d = a.d;
    if (pl.nsplit > 1) VD_REQUIRE(d.ws != nullptr, "vd_conv3x3_ups_phase_f16: split_k=%d needs a workspace", pl.nsplit);
    if (d.out_stats != nullptr && pl.stat_rows == 0) {
        vd_set_error("vd_conv3x3_ups_phase_f16: out_stats requested but the planned launch cannot emit statistics (vd_conv3x3_ups_phase_plan)");
        return VD_ERR_UNSUPPORTED;
    }
    VD_REQUIRE(((size_t)d.out_stats & 7) == 0, "vd_conv3x3_ups_phase_f16: out_stats must be 8-byte aligned");
    VD_REQUIRE(d.stat_sums == nullptr || (d.out_stats != nullptr && ((size_t)d.stat_sums & 7) == 0 && d.M % d.stat_img_rows == 0),
               "vd_conv3x3_ups_phase_f16: stat_sums rides on out_stats (8-byte aligned, whole images of stat_img_rows rows)");
    a.stat_rows = d.out_stats ? pl.stat_rows : 0;
    a.nt_store = 1;
    {   // which operand an XCD keeps in its private L2 (as vd_gemm_f16; the weights here are the four phase matrices)
        const double wbytes = (double)c.g.w_bytes, abytes = (double)a.a0_bytes;
        const int tiles_m = c.g.tiles_m, tiles_n = c.g.tiles_n;
        const double runs = (double)tiles_m * tiles_n / 8.0;
        const double nfast = 8.0 * wbytes * (runs < tiles_n ? runs / tiles_n : 1.0) + abytes * (runs < tiles_n ? tiles_n / runs : 1.0);
        const double mfast = 8.0 * abytes * (runs < tiles_m ? runs / tiles_m : 1.0) + wbytes * (runs < tiles_m ? tiles_m / runs : 1.0);
        a.mfast = mfast < 0.8 * nfast ? 1 : 0;
    }
    c.g.d.out_stats = d.out_stats;
    c.g.d.stat_sums = d.stat_sums;
    c.g.d.sync = nullptr;
    c.g.stat_rows = a.stat_rows;
    c.g.nt_store = a.nt_store;
    c.g.mfast = a.mfast;
    c.g.xcd_local = 0;
    int rc;
    switch (pl.variant) {
#define X(v, BM, BN, WM, WN, NT) \
    case v: rc = launch_conv_halo<BM, BN, WM, WN, NT, 2, false, 4>(c, pl.nsplit, stream); break;
        VD_PHASE_VARIANTS(X)
#undef X
        default: rc = VD_ERR_UNSUPPORTED; break;
    }
    if (rc != VD_OK) return rc;
    return pl.nsplit > 1 ? vd_gemm_launch_reduce(&a, pl.nsplit, stream) : VD_OK;
}
