"""Record what the host-side GEMM / convolution planner answers over a grid of descriptors.

    VD_HIP_LIB=<library of the PARENT commit> python tools/gen_plan_grid.py            # -> tests/golden/gemm_plan_grid.npz
    python tools/gen_plan_grid.py --out replay.npz                                      # the same grid, any library

Planning entry points only (vd_gemm_plan, vd_gemm_stat_rows, vd_gemm_row_sums_ok, vd_gemm_skip_ok, vd_gemm_workspace_bytes,
vd_conv3x3_wstream_supported / _plan, vd_gemm_wstream_supported / _plan): nothing is launched, no GPU is needed.  The recording runs
in a fresh child process without the planner's environment switches, against the library VD_HIP_LIB names (default: the product
library).  tests/test_gemm_planner_cpu.py::test_plan_grid_matches_the_recorded_planner replays the grid against the current library
and compares every array; the committed fixture is generated from a build of the commit BEFORE a planner refactor, never after it.

The grid: every (M, N, K, ksize, epilogue class) row of the per-shape tables under profiles/, a cross product of plain matrices and
one of 3x3 convolutions, each under the variants the planner looks at (epilogue, workspace, counters, split factor, batch,
two-source A, upsampling / stride, folded skip, statistics rows, halo setting, tile override), with an empty tuned table and
with three installed entries.  Combinations the planner cannot tell apart (the halo setting of a plain matrix, ...) are left out.
"""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import zipfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_plan_grid.npz")
SCRUB = ("VD_GEMM_TILE", "VD_CONV_HALO", "VD_WSK", "VD_WSK_MIN_BLOCKS", "VD_HALO_ABL", "VD_GEMM_TUNE")
PROFILES = ("r06_forward_per_shape.txt", "r06_dual_per_shape.txt", "r06_i2v_per_shape.txt", "r06_triple_per_shape.txt")

PTR = 4096                       # a non-null, aligned operand "pointer": the planner never dereferences operands
ACT_GEGLU = 1
BIAS, ROWVEC, RESIDUAL, OUT_F32, LNFOLD, LN_INLOOP = 1, 2, 4, 16, 32, 64
NCFG, NHALO = 27, 13
# tuned table of the second pass: one plain entry, one 3x3 entry, one with a split (M, N, K, ksize, class, tile, split)
TUNED = ((2048, 1280, 1280, 1, 0, 0, 0), (8192, 640, 5760, 3, 0, 1, 1), (2048, 1280, 5120, 1, 0, 1, 4))


def flag_values():
    """the flag bits by name, read from include/vd_hip.h so the grid cannot drift from the ABI"""
    text = open(os.path.join(ROOT, "include", "vd_hip.h")).read()
    out = {}
    for name in ("VD_EPI_BIAS", "VD_EPI_ROWVEC", "VD_EPI_RESIDUAL", "VD_EPI_OUT_F32", "VD_EPI_LNFOLD", "VD_EPI_LN_INLOOP", "VD_ACT_GEGLU"):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


# ---- descriptors ------------------------------------------------------------------------------------------------------------
def epilogues():
    """(act, flags, extra fields) of the epilogue variants of a plain matrix"""
    return [(0, 0, {}), (ACT_GEGLU, 0, {}), (0, RESIDUAL, {"res": PTR}), (0, ROWVEC, {"rowvec": PTR, "rows_per_batch": 64}),
            (0, OUT_F32, {}), (0, LNFOLD, {"colsum": PTR, "ln_stats": PTR}), (0, LNFOLD | LN_INLOOP, {"colsum": PTR}),
            (ACT_GEGLU, LNFOLD, {"colsum": PTR, "ln_stats": PTR}), (ACT_GEGLU, RESIDUAL, {"res": PTR})]


WS_SYNC = ((0, 0), (PTR, 0), (PTR, PTR))
SPLITS = (0, 2, 5, 40)
OVERRIDES = (0, 1, 2, 3, 4, 7, 13, 14, 15)   # the slots vd_gemm_set_override accepts (record() asserts each one is taken)
HALOS = (-1, 0, 3, 6, 13)                    # planner, off, forced variant k - 1 for the accepted k (likewise)


def plain_variants(M, N, K, rows):
    base = {"M": M, "N": N, "K": K, "a0": PTR, "w": PTR, "out": PTR}

    def add(act=0, flags=0, extra=None, ws=0, sync=0, split=0, batch=0, ov=-1, **kw):
        d = dict(base, act=act, flags=flags, ws=ws, sync=sync, split_k=split, batch=batch, _ov=ov, _halo=-1)
        if extra:
            d.update(extra)
        d.update(kw)
        rows.append(d)

    for act, flags, extra in epilogues():
        for ws, sync in WS_SYNC:
            for split in SPLITS:
                for batch in ((1, 3) if split in (0, 2) else (1,)):
                    add(act, flags, extra, ws, sync, split, batch)
    for act, flags, extra in ((0, 0, {}), (ACT_GEGLU, 0, {}), (0, LNFOLD, {"colsum": PTR, "ln_stats": PTR})):
        for split in (0, 2):
            for ov in OVERRIDES:
                add(act, flags, extra, PTR, 0, split, 1, ov)
    for c1 in (64, 320):                       # two-source A: K = c0 + c1
        if K - c1 > 0:
            for act, flags, extra in ((0, 0, {}), (0, RESIDUAL, {"res": PTR}), (ACT_GEGLU, 0, {})):
                for split in (0, 2):
                    add(act, flags, extra, PTR, 0, split, 1, a1=PTR, c0=K - c1, c1=c1)
    img = 64 if M % 64 == 0 else M             # rows of one sample for the emitted statistics
    for act, flags, extra in ((0, 0, {}), (0, RESIDUAL, {"res": PTR}), (0, OUT_F32, {})):
        for ws, sync in ((0, 0), (PTR, 0), (PTR, PTR), (0, PTR)):
            for split in (0, 5):
                add(act, flags, extra, ws, sync, split, 1, stat_img_rows=img)


def conv_variants(B, side, c0, N, rows):
    def geom(ups=0, stride=1, c1=0):
        ho = (side << ups) // stride
        return {"M": B * ho * ho, "N": N, "K": 9 * (c0 + c1), "a0": PTR, "w": PTR, "out": PTR, "Hin": side, "Win": side, "Hout": ho, "Wout": ho,
                "ksize": 3, "stride": stride, "pad": 1, "ups": ups, "c0": c0}

    def add(g, act=0, flags=0, extra=None, ws=0, sync=0, split=0, batch=0, ov=-1, halo=-1, **kw):
        d = dict(g, act=act, flags=flags, ws=ws, sync=sync, split_k=split, batch=batch, _ov=ov, _halo=halo)
        if extra:
            d.update(extra)
        d.update(kw)
        rows.append(d)

    epi = ((0, 0, {}), (0, RESIDUAL, {"res": PTR}), (0, OUT_F32, {}))
    for ups, stride in ((0, 1), (1, 1), (0, 2)):
        g = geom(ups, stride)
        for act, flags, extra in (epi if (ups, stride) == (0, 1) else epi[:2]):
            for ws, sync in WS_SYNC:
                for split in SPLITS:
                    for halo in (HALOS if (ups, stride) == (0, 1) else (-1, 0)):
                        add(g, act, flags, extra, ws, sync, split, 1, halo=halo)
    g = geom()
    for split in (0, 2):
        for halo in (-1, 0):
            add(g, ws=PTR, split=split, batch=3, halo=halo)
            add(g, ACT_GEGLU, ws=PTR, split=split, halo=halo)
            add(g, 0, ROWVEC, {"rowvec": PTR, "rows_per_batch": side * side}, ws=PTR, split=split, halo=halo)
    for c1 in (64, 320):
        g1 = geom(c1=c1)
        for act, flags, extra in epi[:2]:
            for split in (0, 2):
                for halo in (-1, 0, 3):
                    add(g1, act, flags, extra, PTR, 0, split, 1, halo=halo, a1=PTR, c1=c1)
    for sc0 in (100, 320, 1280):               # folded 1x1 skip convolution
        for sc1 in (0, 640):
            skip = {"skip_a0": PTR, "skip_w": PTR, "skip_c0": sc0}
            if sc1:
                skip.update(skip_a1=PTR, skip_c1=sc1)
            for ws in (0, PTR):
                for split in (0, 2):
                    for halo in HALOS[:4] + (13,):
                        add(g, ws=ws, split=split, batch=1, halo=halo, **skip)
                    add(geom(ups=1), ws=ws, split=split, batch=1, **skip)
    for act, flags, extra in epi[:2]:
        for ws, sync in WS_SYNC:
            for split in (0, 5):
                for halo in (-1, 0):
                    add(g, act, flags, extra, ws, sync, split, 1, halo=halo, stat_img_rows=side * side)
    for ov in OVERRIDES:
        for halo in (-1, 0):
            for split in (0, 2):
                add(g, ws=PTR, split=split, batch=1, ov=ov, halo=halo)


def profile_shapes():
    """(M, N, K, ksize, class) of every GEMM / convolution row of the per-shape tables"""
    seen = []
    for name in PROFILES:
        for line in open(os.path.join(ROOT, "profiles", name)):
            m = re.search(r"(\S+) M=(\d+) N=(\d+) K=(\d+)(?: ks=(\d) cls=(\d))?", line)
            if not m:
                continue
            M, N, K = int(m.group(2)), int(m.group(3)), int(m.group(4))
            ks = int(m.group(5)) if m.group(5) else (3 if "conv3x3" in line else 1)
            key = (M, N, K, ks, int(m.group(6) or 0))
            if key not in seen:
                seen.append(key)
    return seen


def profile_variants(M, N, K, ks, cls, rows):
    if ks == 3:
        for B in (8, 4, 16, 12, 24, 2, 6, 3, 1, 18, 9, 36, 32, 48, 64):    # the CFG batches of the measured workloads, most likely first
            side = int(round((M / B) ** 0.5))
            if side in (8, 16, 24, 32, 64) and B * side * side == M:
                conv_variants(B, side, K // 9, N, rows)
                return
        raise AssertionError("no image geometry for M=%d" % M)
    plain_variants(M, N, K, rows)
    if cls & 4:                                        # measured with a two-source A (skip concatenation): the halves as sources
        for split in (0, 2):
            rows.append({"M": M, "N": N, "K": K, "a0": PTR, "a1": PTR, "w": PTR, "out": PTR, "ws": PTR, "c0": K // 2, "c1": K // 2,
                         "split_k": split, "act": ACT_GEGLU if cls & 1 else 0, "_ov": -1, "_halo": -1})


def descriptors():
    """-> (numpy structured array of VdGemmDesc, halo setting per row, tile override per row)"""
    sys.path.insert(0, os.path.join(ROOT, "versatile-diffusion_amd"))
    from vd_hip.loader import VdGemmDesc
    rows = []
    for key in profile_shapes():
        profile_variants(*key, rows)
    for M in (8, 64, 96, 128, 512, 2048, 4096, 8192, 16384, 32768):
        for N in (4, 64, 100, 320, 640, 960, 1280, 1920, 2560, 5120, 10240):
            for K in (12, 64, 320, 640, 1280, 2560, 5120, 10240):
                plain_variants(M, N, K, rows)
    for side in (8, 16, 32, 64, 24):
        for B in (1, 2, 4, 8):
            for c0 in (64, 100, 128, 192, 320, 640, 1280, 2560):
                for N in sorted({c0, 640}):
                    conv_variants(B, side, c0, N, rows)
    used = set().union(*(r.keys() for r in rows)) - {"_ov", "_halo"}
    arr = np.zeros(len(rows), dtype=np.dtype(VdGemmDesc))
    assert used <= set(arr.dtype.names), used - set(arr.dtype.names)
    arr["alpha"] = 1.0
    for f in sorted(used):
        arr[f] = [r.get(f, 0) for r in rows]
    halo = np.array([r["_halo"] for r in rows], dtype=np.int8)
    ov = np.array([r["_ov"] for r in rows], dtype=np.int8)
    return arr, halo, ov


# ---- recording --------------------------------------------------------------------------------------------------------------
def record():
    sys.path.insert(0, os.path.join(ROOT, "versatile-diffusion_amd"))
    from vd_hip import loader
    fl = flag_values()
    assert (fl["VD_EPI_BIAS"], fl["VD_EPI_ROWVEC"], fl["VD_EPI_RESIDUAL"], fl["VD_EPI_OUT_F32"], fl["VD_EPI_LNFOLD"], fl["VD_EPI_LN_INLOOP"], fl["VD_ACT_GEGLU"]) == \
        (BIAS, ROWVEC, RESIDUAL, OUT_F32, LNFOLD, LN_INLOOP, ACT_GEGLU), fl
    h = ctypes.CDLL(loader.lib_path())          # a handle of its own: descriptors are passed by address
    P, I, IP = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    for name, res, args in (("vd_gemm_plan", I, [P, IP, IP]), ("vd_gemm_stat_rows", I, [P, IP]), ("vd_gemm_row_sums_ok", I, [P]),
                            ("vd_gemm_skip_ok", I, [P]), ("vd_gemm_workspace_bytes", ctypes.c_size_t, [P]),
                            ("vd_conv3x3_wstream_supported", I, [P]), ("vd_conv3x3_wstream_plan", I, [P, IP]),
                            ("vd_gemm_wstream_supported", I, [P]), ("vd_gemm_wstream_plan", I, [P, IP]),
                            ("vd_last_error", ctypes.c_char_p, []), ("vd_gemm_config_name", ctypes.c_char_p, [I]),
                            ("vd_gemm_num_configs", I, []), ("vd_gemm_set_override", I, [I]), ("vd_conv_halo_set_variant", I, [I]),
                            ("vd_gemm_tune_set", I, [I] * 7), ("vd_gemm_tune_clear", I, [])):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, args
    out = {}
    out["num_configs"] = np.array([h.vd_gemm_num_configs()], dtype=np.int32)
    out["config_names"] = np.array([(h.vd_gemm_config_name(i) or b"") for i in range(NCFG + NHALO + 1)])
    out["override_accepts"] = np.array([h.vd_gemm_set_override(i) == 0 for i in range(-1, NCFG + 2)], dtype=np.int8)
    h.vd_gemm_set_override(-1)
    out["halo_accepts"] = np.array([h.vd_conv_halo_set_variant(i) == 0 for i in range(-2, NHALO + 2)], dtype=np.int8)
    h.vd_conv_halo_set_variant(-1)
    arr, halo, ov = descriptors()
    n, size, base = len(arr), arr.dtype.itemsize, arr.ctypes.data
    out["n_descriptors"] = np.array([n], dtype=np.int64)
    out["descriptor_crc"] = np.array([zlib.crc32(arr.tobytes()), zlib.crc32(halo.tobytes()), zlib.crc32(ov.tobytes())], dtype=np.uint32)
    ks3 = arr["ksize"] == 3
    has_skip = arr["skip_a0"] != 0
    key = set((t[0], t[1], t[2], t[3]) for t in TUNED)
    tuned_rows = np.array([i for i in range(n) if i % 16 == 0 or (int(arr["M"][i]), int(arr["N"][i]), int(arr["K"][i]), max(int(arr["ksize"][i]), 1)) in key], dtype=np.int64)
    out["n_tuned_rows"] = np.array([len(tuned_rows)], dtype=np.int64)
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    ra, rb = ctypes.byref(a), ctypes.byref(b)
    crc, err = zlib.crc32, h.vd_last_error

    def run(idx, tag):
        m = len(idx)
        plan = np.zeros((m, 3), dtype=np.int16)       # return code, tile_cfg, nsplit
        stat = np.zeros((m, 2), dtype=np.int16)       # return code, rows
        oks = np.full((m, 2), -1, dtype=np.int8)      # row_sums_ok, skip_ok (-1: no skip fields)
        errs = np.zeros((m, 2), dtype=np.uint32)      # crc32 of vd_last_error() of a failing plan / stat_rows
        wsb = np.zeros(m, dtype=np.int64)
        wst = np.full((m, 3), -1, dtype=np.int16)     # conv wstream: supported, plan rc, plan split | gemm wstream: supported, 0, split
        cur_h, cur_o = -1, -1
        for j, i in enumerate(idx):
            i = int(i)
            p = base + i * size
            if halo[i] != cur_h:
                cur_h = int(halo[i])
                assert h.vd_conv_halo_set_variant(cur_h) == 0, cur_h
            if ov[i] != cur_o:
                cur_o = int(ov[i])
                assert h.vd_gemm_set_override(cur_o) == 0, cur_o
            a.value, b.value = -7, -7
            rc = h.vd_gemm_plan(p, ra, rb)
            plan[j] = (rc, a.value, b.value)
            if rc:
                errs[j, 0] = crc(err())
            a.value = -7
            rc = h.vd_gemm_stat_rows(p, ra)
            stat[j] = (rc, a.value)
            if rc:
                errs[j, 1] = crc(err())
            oks[j, 0] = h.vd_gemm_row_sums_ok(p)
            if has_skip[i]:
                oks[j, 1] = h.vd_gemm_skip_ok(p)
            wsb[j] = h.vd_gemm_workspace_bytes(p)
            if ks3[i]:
                s = h.vd_conv3x3_wstream_supported(p)
                wst[j, 0] = s
                if s:                                  # the plan of an unsupported geometry is undefined (no tiles to divide by)
                    a.value = -7
                    wst[j, 1] = h.vd_conv3x3_wstream_plan(p, ra)
                    wst[j, 2] = a.value
            else:
                s = h.vd_gemm_wstream_supported(p)
                wst[j, 0] = s
                if s:
                    a.value = -7
                    wst[j, 1] = h.vd_gemm_wstream_plan(p, ra)
                    wst[j, 2] = a.value
        h.vd_conv_halo_set_variant(-1)
        h.vd_gemm_set_override(-1)
        for name, v in (("plan", plan), ("stat_rows", stat), ("ok", oks), ("err_crc", errs), ("workspace_bytes", wsb), ("wstream", wst)):
            out[tag + name] = np.ascontiguousarray(v.T)   # one field after the other: compresses several times better

    h.vd_gemm_tune_clear()
    run(np.arange(n), "")
    for t in TUNED:
        assert h.vd_gemm_tune_set(*t) == 0, t
    run(tuned_rows, "tuned_")
    h.vd_gemm_tune_clear()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:
        env = {k: v for k, v in os.environ.items() if k not in SCRUB}
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__), "--child", "--out", args.out], env=env))
    out = record()
    with zipfile.ZipFile(args.out, "w", zipfile.ZIP_LZMA) as z:   # an .npz numpy.load reads; LZMA: the arrays repeat over long distances
        for name, v in out.items():
            info = zipfile.ZipInfo(name + ".npy")   # (no time stamp: the same answers give the same file)
            info.compress_type = zipfile.ZIP_LZMA
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, v, allow_pickle=False)
    print("%d descriptors (+ %d with the tuned table), %d bytes -> %s" % (out["n_descriptors"][0], out["n_tuned_rows"][0], os.path.getsize(args.out), args.out))


if __name__ == "__main__":
    main()
