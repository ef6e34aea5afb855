"""Windowed (MultiDiffusion) sampling on the GPU: the gather and merge kernels against torch indexing and the restated chain of
tests/window_cases.py, the windowed forward (the samplers' _eps) against the fp32 oracle run per window and merged, the
samplers' windowed loops against oracle loops, and the plumbing: graph replay, kept graphs keyed by the geometry, window ==
canvas, inpainting, the guidance rescale, seeded SDE noise and the sharding helper."""
import ctypes

import numpy as np
import pytest
import torch

import deepcache_cases as dc
import window_cases as wc
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg
from window_cases import FWD_TOL, LATENT_TOL

pytestmark = pytest.mark.gpu

# (H, W, window, stride, wrap): the 12 x 20 canvas with and without wrap-around, and one odd geometry whose rows are neither
# a multiple of 8 elements nor 16-byte aligned
GEOS = [(12, 20, (8, 8), (4, 4), False), (12, 20, (8, 8), (4, 4), True), (12, 20, (8, 8), (8, 6), False),
        (12, 20, (8, 8), (8, 6), True), (9, 13, (5, 7), (3, 3), False), (9, 13, (5, 7), (3, 3), True)]
GEO_IDS = ["%dx%d-w%dx%d-s%dx%d-%s" % (H, W, h, w, sy, sx, "wrap" if wr else "flat") for H, W, (h, w), (sy, sx), wr in GEOS]


@pytest.fixture(scope="module")
def tiny(dev):
    from lib.model_zoo import get_model
    m = meta()
    net = get_model()(tiny_vd_cfg(m), verbose=False)
    sd = synth_into(net, m["seed"])
    net = net.half()
    net.to(dev)
    return net, sd


@pytest.fixture(scope="module")
def plan():
    from oracle import vd_oracle as O
    return O.unet_plan(**meta()["unet2d"])


def _dev_tables(geo, dev):
    return (torch.from_numpy(geo["offs"]).to(dev), torch.from_numpy(geo["wgt"]).to(dev), torch.from_numpy(geo["inv_den"]).to(dev))


# ---- 1. gather -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geo", GEOS, ids=GEO_IDS)
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("B", [1, 3])
def test_gather_is_torch_indexing_bitwise(dev, B, C, geo):
    from vd_hip import ops
    H, W, (h, w), stride, wrap = geo
    g = wc.geometry(H, W, (h, w), stride, wrap)
    x = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(B * 100 + C)).half()
    ref = wc.gather_ref(x, g["offs"], h, w, wrap)
    offs = torch.from_numpy(g["offs"]).to(dev)
    out = ops.window_gather(x.to(dev), offs, h, w, wrap)
    assert out.dtype == torch.float16 and tuple(out.shape) == (B, len(g["offs"]), C, h, w)
    assert torch.equal(out.cpu(), ref)
    # a canvas and a window buffer that start 2 bytes past a 16-byte boundary: the same elements through other accesses
    xs = torch.empty(x.numel() + 1, dtype=torch.float16, device=dev)[1:].view(x.shape)
    xs.copy_(x)
    buf = torch.full((ref.numel() + 1,), float("nan"), dtype=torch.float16, device=dev)
    res = ops.window_gather(xs, offs, h, w, wrap, out=buf[1:].view(ref.shape))
    assert res.data_ptr() == buf.data_ptr() + 2 and torch.equal(res.cpu(), ref)
    assert bool(torch.isnan(buf[0]))                                   # nothing in front of the buffer was written


# ---- 2. merge --------------------------------------------------------------------------------------------------------------

def _eps_win(rows, Wn, C, h, w, seed):
    return torch.randn((rows, Wn, C, h, w), generator=torch.Generator().manual_seed(seed)).half()


@pytest.mark.parametrize("geo", GEOS, ids=GEO_IDS)
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("B,guided", [(1, False), (3, True), (1, True)])
def test_merge_uniform_is_the_restated_chain_bitwise(dev, B, guided, C, geo):
    from vd_hip import ops
    H, W, (h, w), stride, wrap = geo
    g = wc.geometry(H, W, (h, w), stride, wrap)
    rows = (2 if guided else 1) * B
    e = _eps_win(rows, len(g["offs"]), C, h, w, 7 * rows + C)
    offs, wgt, inv = _dev_tables(g, dev)
    out = ops.window_merge(e.to(dev), offs, wgt, inv, H, W, len(g["offs"]), wrap, True, True)
    assert out.dtype == torch.float16 and tuple(out.shape) == (rows, C, H, W)
    assert torch.equal(out.cpu(), wc.merge_restated(e, g["offs"], g["wgt"], g["inv_den"], H, W, wrap))


@pytest.mark.parametrize("geo", GEOS, ids=GEO_IDS)
def test_merge_gaussian_within_one_fp16_rounding_of_the_exact_value(dev, geo):
    """|out - ref64| <= 2^-11 |ref64| + 2^-24 per element: one fp16 rounding of the exact value plus the fp32 chain's slack."""
    from vd_hip import ops
    H, W, (h, w), stride, wrap = geo
    g = wc.geometry(H, W, (h, w), stride, wrap, weight="gaussian")
    e = _eps_win(4, len(g["offs"]), 4, h, w, 11)
    offs, wgt, inv = _dev_tables(g, dev)
    out = ops.window_merge(e.to(dev), offs, wgt, inv, H, W, len(g["offs"]), wrap, True, True).cpu().double()
    ref = wc.merge_ref64(e, g["offs"], g["wgt"], g["inv_den"], H, W, wrap)
    excess = (out - ref).abs() - (2.0 ** -11 * ref.abs() + 2.0 ** -24)
    print("gaussian merge: max |out - ref64| %.3e, max excess over the bound %.3e" % (float((out - ref).abs().max()), float(excess.max())))
    assert bool(torch.isfinite(out).all()) and float(excess.max()) <= 0.0


def test_merge_without_overlap_keeps_the_windows_bits(dev):
    from vd_hip import ops
    g = wc.geometry(16, 24, (8, 8), (8, 8))
    assert len(g["offs"]) == 6 and np.all(g["inv_den"] == 1.0)
    e = _eps_win(2, 6, 4, 8, 8, 3)
    offs, wgt, inv = _dev_tables(g, dev)
    out = ops.window_merge(e.to(dev), offs, wgt, inv, 16, 24, 6, False, True, True).cpu()
    for k, (oy, ox) in enumerate(g["offs"]):
        assert torch.equal(out[:, :, oy:oy + 8, ox:ox + 8], e[:, k])


@pytest.mark.parametrize("weight", ["uniform", "gaussian"])
@pytest.mark.parametrize("wrap", [False, True])
def test_merge_has_the_same_bits_however_the_windows_are_chunked(dev, weight, wrap):
    """Eight windows as 1, 2, 3 and 8 launches; the padded slots of the last launch hold NaN and repeat the last window's
    offsets, as the samplers' tables do: they are never read."""
    from lib.model_zoo import windows
    from vd_hip import ops
    H, W, h, w = 12, 16 if wrap else 20, 8, 8
    g = wc.geometry(H, W, (h, w), (4, 4), wrap, weight)
    n = len(g["offs"])
    assert n == 8
    e = _eps_win(4, n, 3, h, w, 5)
    _, wgt, inv = _dev_tables(g, dev)
    outs = []
    for batch in (8, 4, 3, 1):
        nc, m = windows.window_chunks(n, batch)
        assert (nc, m) == {8: (1, 8), 4: (2, 4), 3: (3, 3), 1: (8, 1)}[batch]
        offs = np.concatenate([g["offs"], np.repeat(g["offs"][-1:], nc * m - n, 0)]).reshape(nc, m, 2)
        ep = torch.full((4, nc * m, 3, h, w), float("nan"), dtype=torch.float16)
        ep[:, :n] = e
        acc = torch.full((4, 3, H, W), float("nan"), dtype=torch.float32, device=dev)      # never read by the first launch
        out = torch.full((4, 3, H, W), float("nan"), dtype=torch.float16, device=dev)
        for k in range(nc):
            chunk = ep[:, k * m:(k + 1) * m].contiguous().to(dev)
            ret = ops.window_merge(chunk, torch.from_numpy(offs[k]).to(dev), wgt, inv, H, W, min(m, n - k * m), wrap, k == 0,
                                   k == nc - 1, acc=acc if nc > 1 else None, out=out)
            assert ret is (out if k == nc - 1 else acc)
            assert k == nc - 1 or bool(torch.isnan(out).all())          # eps is written by the last launch only
        assert bool(torch.isfinite(out).all())
        outs.append(out.cpu())
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    if weight == "uniform":
        assert torch.equal(outs[0], wc.merge_restated(e, g["offs"], g["wgt"], g["inv_den"], H, W, wrap))


def test_entry_points_refuse_bad_arguments(dev):
    from vd_hip import ops
    from vd_hip.loader import VdHipError, lib
    L = lib()
    f16 = dict(device=dev, dtype=torch.float16)
    x, win = torch.zeros((1, 2, 8, 12), **f16), torch.zeros((1, 2, 2, 8, 8), **f16)
    offs = torch.zeros((2, 2), device=dev, dtype=torch.int32)
    wgt, inv = torch.ones((8, 8), device=dev), torch.ones((8, 12), device=dev)
    acc, eps = torch.zeros((1, 2, 8, 12), device=dev), torch.zeros((1, 2, 8, 12), **f16)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def gather(x=x, win=win, offs=offs, B=1, C=2, H=8, W=12, h=8, w=8, slots=2, wrap=0):
        return L.vd_window_gather_f16(P(x), P(win), P(offs), B, C, H, W, h, w, slots, wrap, stream)

    def merge(e=win, acc=acc, eps=eps, wgt=wgt, inv=inv, offs=offs, RB=1, C=2, H=8, W=12, h=8, w=8, slots=2, valid=2, wrap=0,
              first=1, last=1):
        return L.vd_window_merge_f16(P(e), P(acc), P(eps), P(wgt), P(inv), P(offs), RB, C, H, W, h, w, slots, valid, wrap, first,
                                     last, stream)

    assert gather() == 0 and merge() == 0 and merge(acc=None) == 0 and merge(first=1, last=0, eps=None) == 0
    bad_gather = [dict(x=None), dict(win=None), dict(offs=None), dict(B=0), dict(C=0), dict(H=0), dict(W=-1), dict(h=0), dict(w=0),
                  dict(slots=0), dict(h=9), dict(w=13)]
    for kw in bad_gather:
        assert gather(**kw) < 0 and L.vd_last_error().decode().startswith("vd_window_gather_f16"), kw
    bad_merge = [dict(e=None), dict(wgt=None), dict(inv=None), dict(offs=None), dict(eps=None), dict(acc=None, last=0),
                 dict(acc=None, first=0), dict(RB=0), dict(C=-2), dict(H=0), dict(W=0), dict(h=0), dict(w=0), dict(slots=0),
                 dict(h=9), dict(w=13), dict(valid=0), dict(valid=3), dict(valid=-1)]
    for kw in bad_merge:
        assert merge(**kw) < 0 and L.vd_last_error().decode().startswith("vd_window_merge_f16"), kw
    # the wrappers check shape, dtype and device before the library is called
    for call in (lambda: ops.window_gather(x.float(), offs, 8, 8, False), lambda: ops.window_gather(x.cpu(), offs, 8, 8, False),
                 lambda: ops.window_gather(x, offs.long(), 8, 8, False), lambda: ops.window_gather(x, offs.view(-1), 8, 8, False),
                 lambda: ops.window_gather(x, offs, 9, 8, False), lambda: ops.window_gather(x[0], offs, 8, 8, False),
                 lambda: ops.window_gather(x, offs, 8, 8, False, out=win[:, :1]),
                 lambda: ops.window_gather(x.transpose(2, 3), offs, 8, 8, False),
                 lambda: ops.window_merge(win, offs, wgt, inv, 8, 12, 3, False, True, True),
                 lambda: ops.window_merge(win, offs, wgt, inv, 8, 12, 0, False, True, True),
                 lambda: ops.window_merge(win, offs, wgt.half(), inv, 8, 12, 2, False, True, True),
                 lambda: ops.window_merge(win, offs, wgt, inv[:, :8].contiguous(), 8, 12, 2, False, True, True),
                 lambda: ops.window_merge(win, offs, wgt[:4].contiguous(), inv, 8, 12, 2, False, True, True),
                 lambda: ops.window_merge(win, offs[:1], wgt, inv, 8, 12, 1, False, True, True),
                 lambda: ops.window_merge(win[0], offs, wgt, inv, 8, 12, 2, False, True, True),
                 lambda: ops.window_merge(win, offs, wgt, inv, 8, 12, 2, False, False, True),
                 lambda: ops.window_merge(win, offs, wgt, inv, 8, 12, 2, False, True, True, acc=acc.half()),
                 lambda: ops.window_merge(win, offs, wgt, inv, 8, 12, 2, False, True, True, out=eps[:, :1]),
                 lambda: ops.window_merge(win.cpu(), offs, wgt, inv, 8, 12, 2, False, True, True)):
        with pytest.raises(VdHipError):
            call()


# ---- 3. the windowed forward -----------------------------------------------------------------------------------------------

def _ci(c, u, scale, ctype="text", **kw):
    return dict({"type": ctype, "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale},
                **kw)


def _on_dev(c, dev):
    return dict(c, conditioning=c["conditioning"].half().to(dev),
                unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))


def _fwd_inputs(seed, B, H, W, dual):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, H, W), generator=g).half().float()             # fp16 values: the device sees the oracle's inputs
    r = lambda L: (torch.randn((B, L, 128), generator=g) * 0.5).half().float()
    cs = [_ci(r(77), r(77), None, ratio=0.4 if dual else 1.0)]
    if dual:
        cs.append(_ci(r(50), r(50), None, "image", ratio=0.6))
    return x, cs


def _windowed_forward(net, dev, x, cs, scale, t, keys):
    """The sampler's own _eps, eagerly, on the canvas x: the plan, its device state and the context batches as a call makes them."""
    from lib.model_zoo.ddim import DDIMSampler, _window_args
    s = DDIMSampler(net)
    x_info = dict({"type": "image"}, **keys)
    wplan = _window_args(x_info, list(x.shape), net)
    cis, guided, _, _ = s._cfg_contexts([_on_dev(dict(c, unconditional_guidance_scale=scale), dev) for c in cs], wplan["m"])
    for ci in cis:
        ci["kv_cache"] = {}
    xd = x.half().to(dev)
    rows = (2 if guided else 1) * x.shape[0]
    ts = torch.full((rows * wplan["m"],), t, dtype=torch.long, device=dev)
    eps = s._eps(x_info, xd, ts, cis, guided, len(cs) == 1, window=s._window_state(wplan, xd, guided))
    assert eps.dtype == torch.float16 and tuple(eps.shape) == (rows,) + tuple(x.shape[1:])
    return eps.clone(), wplan


# B, guided, H, W, window, stride, wrap, dual, window_batch, weight
FWD_CASES = {"B2-guided-12x20": (2, True, 12, 20, 8, (4, 4), False, False, 8, "uniform"),
             "B1-unguided-8x20": (1, False, 8, 20, 8, (8, 6), False, False, 8, "uniform"),
             "B3-guided-wrap-8x24": (3, True, 8, 24, 8, (8, 4), True, False, 8, "uniform"),
             "B1-guided-dual-8x20": (1, True, 8, 20, 8, (8, 6), False, True, 8, "uniform"),
             "B2-guided-12x20-batch1": (2, True, 12, 20, 8, (4, 4), False, False, 1, "uniform"),
             "B2-guided-12x20-batch3": (2, True, 12, 20, 8, (4, 4), False, False, 3, "uniform"),
             "B2-guided-12x20-gaussian-batch3": (2, True, 12, 20, 8, (4, 4), False, False, 3, "gaussian")}


@pytest.mark.parametrize("case", list(FWD_CASES))
def test_windowed_forward_vs_the_oracle_per_window(tiny, plan, dev, case):
    net, sd = tiny
    B, guided, H, W, window, stride, wrap, dual, batch, weight = FWD_CASES[case]
    x, cs = _fwd_inputs(17 + B + H, B, H, W, dual)
    scale = 7.5 if guided else 1.0
    keys = {"window": window, "window_stride": stride, "window_wrap": wrap, "window_batch": batch, "window_weight": weight}
    eps, wplan = _windowed_forward(net, dev, x, cs, scale, 500, keys)
    geo = wc.geometry(H, W, window, stride, wrap, weight)
    assert wplan["n"] == len(geo["offs"]) and wplan["nc"] * wplan["m"] >= wplan["n"]
    xin = torch.cat([x, x]) if guided else x
    t = torch.full((xin.shape[0],), 500, dtype=torch.long)
    ctx = dc.cfg_contexts(cs, guided)
    ref = wc.windowed_eps(sd, plan, xin, t, ctx, geo)
    canvas = dc.walk(sd, plan, xin, t, ctx)
    err, gap = rel_l2(eps, ref), rel_l2(ref, canvas)
    print("%s: %d windows as %d x %d; rel-L2 vs the windowed oracle %.3e; windowed oracle vs its plain canvas forward %.3e"
          % (case, wplan["n"], wplan["nc"], wplan["m"], err, gap))
    assert gap > 2 * FWD_TOL                    # the bound tells the windowed prediction from the plain forward on the canvas
    assert err < FWD_TOL


# ---- 4. loops ----------------------------------------------------------------------------------------------------------------

SHAPE = [2, 4, 12, 20]
KEYS = {"window": 8, "window_stride": 4}


def _case(dev, seed, shape=tuple(SHAPE)):
    g = torch.Generator().manual_seed(seed)
    xT = torch.randn(shape, generator=g).half()
    c = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half()
    u = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half()
    return xT.to(dev), c.to(dev), u.to(dev)


def _make(kind, net, **kw):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from lib.model_zoo.unipc import UniPCSampler
    return {"ddim": DDIMSampler, "2m": DPMSolverSampler, "unipc": UniPCSampler, "sde": DPMSolverSDESampler}[kind](net, **kw)


def _t2i(sampler, xT, c, u, scale, steps, c_keys=None, **keys):
    z, inter = sampler.sample(steps=steps, shape=list(xT.shape), x_info=dict({"type": "image", "xt": xT}, **keys),
                              c_info=_ci(c, u, scale, **(c_keys or {})), verbose=False)
    return z


@pytest.mark.parametrize("kind", ["ddim", "2m", "unipc"])
def test_windowed_loops_vs_oracle_loops(tiny, plan, dev, kind):
    net, sd = tiny
    xT, c, u = _case(dev, 21)
    sampler = _make(kind, net)
    z = _t2i(sampler, xT, c, u, 7.5, 6, **KEYS)
    cs = [_ci(c.float().cpu(), u.float().cpu(), 7.5)]
    geo = wc.geometry(12, 20, 8, 4)
    ref = wc.oracle_loop(sd, plan, sampler, kind, xT.float().cpu(), cs, 7.5, geo)
    plain = dc.oracle_loop(sd, plan, sampler, kind, xT.float().cpu(), cs, 7.5)
    err, gap = rel_l2(z, ref), rel_l2(ref, plain)
    print("%s: final latent rel-L2 vs the windowed oracle loop %.3e; windowed vs plain oracle loop %.3e" % (kind, err, gap))
    assert tuple(z.shape) == tuple(SHAPE) and z.dtype == xT.dtype
    assert gap > 2 * LATENT_TOL                 # the bound tells the windowed loop from the plain loop on the canvas
    assert err < LATENT_TOL


def test_windowed_sde_with_seeds_repeats_and_eta_zero_is_2m(tiny, dev):
    net, _ = tiny
    xT, c, u = _case(dev, 22)
    run = lambda s, **kw: s.sample(steps=6, shape=SHAPE, x_info=dict({"type": "image", "xt": xT, "seeds": [5, 6]}, **KEYS),
                                   c_info=_ci(c, u, 7.5), verbose=False, **kw)[0]
    shared = _make("sde", net)
    z = run(shared)
    assert bool(torch.isfinite(z).all())
    assert torch.equal(run(shared), z) and torch.equal(run(_make("sde", net)), z)
    z0 = run(_make("sde", net), eta=0.)
    assert torch.equal(z0, _t2i(_make("2m", net), xT, c, u, 7.5, 6, **KEYS)) and not torch.equal(z0, z)


# ---- 5. plumbing -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,batch", [("ddim", 8), ("unipc", 3)])
def test_graph_replay_matches_eager_steps_bitwise(tiny, dev, monkeypatch, kind, batch):
    net, _ = tiny
    case = _case(dev, 23)
    z_graph = _t2i(_make(kind, net), *case, 7.5, 6, window_batch=batch, **KEYS)
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _make(kind, net)
    assert not eager.use_graph
    assert torch.equal(z_graph, _t2i(eager, *case, 7.5, 6, window_batch=batch, **KEYS))


def test_window_equal_to_the_canvas_is_the_plain_call(tiny, dev):
    net, _ = tiny
    case = _case(dev, 24)
    s = _make("2m", net)
    z = _t2i(s, *case, 7.5, 6)
    assert torch.equal(_t2i(s, *case, 7.5, 6, window=(12, 20)), z)
    assert torch.equal(_t2i(s, *case, 7.5, 6, window=(12, 20), window_stride=(3, 5), window_weight="gaussian"), z)
    assert len(s._static) == 1 and "window" not in next(iter(s._static.values()))           # one state: the plain one
    assert not torch.equal(_t2i(s, *case, 7.5, 6, **KEYS), z)


def test_kept_graphs_are_keyed_by_the_geometry(tiny, dev):
    """Two window geometries and the plain call alternate on one sampler (which keeps two states, so some calls capture again):
    every call equals a fresh sampler's, whatever ran before it."""
    net, _ = tiny
    a, b = _case(dev, 25), _case(dev, 26)
    geos = [dict(KEYS), dict(KEYS, window_weight="gaussian"), {}, dict(KEYS, window_wrap=True)]
    fresh = [[_t2i(_make("ddim", net), *case, 7.5, 6, **g) for g in geos] for case in (a, b)]
    for i in range(len(geos)):
        for j in range(i):
            assert not torch.equal(fresh[0][i], fresh[0][j]), (i, j)                      # four different computations
    shared = _make("ddim", net)
    for n, gi in enumerate([0, 1, 2, 0, 1, 2, 1, 3]):
        assert torch.equal(_t2i(shared, *(a, b)[n % 2], 7.5, 6, **geos[gi]), fresh[n % 2][gi]), n
    # a second call on the kept graph: replayed, not captured again
    st = list(shared._static.values())[-1]
    graph = st["graph"]
    assert graph is not None and st["window"]["plan"]["key"] == (8, 8, 4, 4, True, "uniform", 2, 5)
    assert torch.equal(_t2i(shared, *a, 7.5, 6, **geos[3]), fresh[0][3]) and list(shared._static.values())[-1]["graph"] is graph
    # ten wrapped windows run as two forwards of five slots: the step's buffers are sized for that batch
    assert tuple(st["ts"].shape) == (2 * 2 * 5,) and tuple(st["c"][0].shape) == (2 * 2 * 5, 77, 128)
    assert tuple(st["window"]["win"].shape) == (2, 5, 4, 8, 8) and tuple(st["window"]["acc"].shape) == (4, 4, 12, 20)
    shared.release_graphs()
    assert shared._static == {}


def test_windowed_inpainting_returns_the_known_region_bitwise(tiny, dev):
    net, _ = tiny
    _, c, u = _case(dev, 27)
    x0 = (torch.randn(SHAPE, generator=torch.Generator().manual_seed(4)) * 0.5).half().to(dev)
    mask = torch.ones((2, 1, 12, 20))
    mask[..., :5, :] = 0                         # keep the top rows, across the first row of windows and into the second
    mask = mask.half().to(dev)
    for kind in ("ddim", "2m"):
        z, _ = _make(kind, net).sample(steps=6, shape=SHAPE, x_info=dict({"type": "image", "x0": x0, "inpaint_mask": mask}, **KEYS),
                                       c_info=_ci(c, u, 7.5), verbose=False)
        keep = (mask == 0).expand_as(x0)
        assert torch.equal(z[keep], x0[keep])
        assert rel_l2(z[~keep], x0[~keep]) > 0.1 and bool(torch.isfinite(z).all())


def test_guidance_rescale_works_on_the_canvas_prediction(tiny, dev, monkeypatch):
    """The factors of every step are ddim.cfg_rescale_factors of the fused, canvas-shaped [e_uncond ; e_cond] of that step
    (within 4 fp32 ulp, test_cfg_rescale_gpu's bound for the factor kernel), and the graph replays the eager steps' bits."""
    from lib.model_zoo.ddim import cfg_rescale_factors
    net, _ = tiny
    case = _case(dev, 28)
    run = lambda s: s.sample(steps=6, shape=SHAPE, x_info=dict({"type": "image", "xt": case[0]}, **KEYS),
                             c_info=_ci(case[1], case[2], 7.5, guidance_rescale=0.7), verbose=False, log_every_t=1)
    z_graph, i_graph = run(_make("2m", net))
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _make("2m", net)
    seen, inner = [], eager._eps

    def recording(*args, **kwargs):
        e = inner(*args, **kwargs)
        if tuple(e.shape[-2:]) == (12, 20):
            seen.append(e.clone())
        return e

    eager._eps = recording
    z, inter = run(eager)
    assert torch.equal(z, z_graph)
    assert len(seen) == len(inter["guidance_rescale"]) == len(i_graph["guidance_rescale"]) == 7
    for e, k, kg in zip(seen, inter["guidance_rescale"], i_graph["guidance_rescale"]):
        assert tuple(e.shape) == (4, 4, 12, 20) and torch.equal(k, kg)
        ref = cfg_rescale_factors(e.cpu(), 7.5, 0.7)
        assert bool(((k.cpu().double() - ref).abs() <= 4 * 2.0 ** -23 * ref.abs()).all()), (k.tolist(), ref.tolist())
    assert not torch.equal(z, _t2i(_make("2m", net), *case, 7.5, 6, **KEYS))


def test_eager_ddim_loop_runs_windowed(tiny, dev):
    """eta > 0 runs DDIM's eager loop on the same _eps: at eta = 0 with the graph off the two loops' kernels differ (host
    scalars against the device row), so the check is the seeded repeat and the distance from the plain call."""
    net, _ = tiny
    xT, c, u = _case(dev, 29)
    outs = []
    for keys in (KEYS, KEYS, {}):
        torch.manual_seed(3)
        outs.append(_make("ddim", net).sample(steps=6, shape=SHAPE, x_info=dict({"type": "image", "xt": xT}, **keys),
                                              c_info=_ci(c, u, 7.5), eta=0.5, verbose=False)[0])
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())
    assert rel_l2(outs[0], outs[2]) > 1e-3


def test_multicontext_call_runs_windowed(tiny, dev):
    net, _ = tiny
    xT, c, u = _case(dev, 30)
    g = torch.Generator().manual_seed(31)
    ci, ui = [(torch.randn((2, 50, 128), generator=g) * 0.5).half().to(dev) for _ in range(2)]
    cs = lambda: [_ci(c, u, 7.5, ratio=0.4), _ci(ci, ui, 7.5, "image", ratio=0.6)]
    run = lambda s, **keys: s.sample_multicontext(steps=6, shape=SHAPE, x_info=dict({"type": "image", "xt": xT}, **keys),
                                                  c_info_list=cs(), verbose=False)[0]
    shared = _make("unipc", net)
    z = run(shared, **KEYS)
    assert torch.equal(run(shared, **KEYS), z) and torch.equal(run(_make("unipc", net), **KEYS), z)
    assert rel_l2(z, run(shared)) > 1e-3 and bool(torch.isfinite(z).all())


def test_sharded_world1_matches_direct_windowed_sample(tiny, dev):
    from lib.model_zoo import sharded
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    gold = load_gold("ddim_tiny.npz")
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dev).half()
    ct = _ci(T(gold["c_text"]), T(gold["u_text"]), 7.5)
    seed, steps = 3, 6
    imgs = sharded.vd_sample_sharded(net, UniPCSampler(net), steps, SHAPE, [dict(ct)], seed, guidance_scale=7.5,
                                     device_generator=True, window=8, window_stride=(4, 6), window_weight="gaussian", window_batch=4)
    torch.manual_seed(seed + 100)
    keys = {"window": 8, "window_stride": (4, 6), "window_weight": "gaussian", "window_batch": 4}
    z, _ = UniPCSampler(net).sample(steps=steps, shape=SHAPE, x_info=dict({"type": "image"}, **keys), c_info=dict(ct), verbose=False)
    assert torch.equal(imgs, net.vae_decode(z, which="image"))
    torch.manual_seed(seed + 100)
    z_plain, _ = UniPCSampler(net).sample(steps=steps, shape=SHAPE, x_info={"type": "image"}, c_info=dict(ct), verbose=False)
    assert not torch.equal(z, z_plain)
