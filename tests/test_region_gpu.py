"""Regional prompts on the windowed path, on the GPU: the masked merge kernel against the restated chain of
tests/region_cases.py and against its sibling ops.window_merge, the regional forward (the samplers' _eps) against the fp32
oracle run per (region, window) and merged in float64, the samplers' regional loops against oracle loops, and the plumbing:
graph replay, one kept graph for every mask of a geometry, R = 1 and window == canvas, seeded SDE noise, inpainting and the
sharding helper."""
import ctypes

import numpy as np
import pytest
import torch

import deepcache_cases as dc
import region_cases as rc
import window_cases as wc
from region_cases import FWD_TOL, LATENT_TOL
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

# (H, W, window, stride, wrap): the 12 x 20 canvas and one odd geometry, flat and wrapped
GEOS = [(12, 20, (8, 8), (4, 4), False), (12, 20, (8, 8), (4, 4), True), (9, 13, (5, 7), (3, 3), False),
        (9, 13, (5, 7), (3, 3), True)]
GEO_IDS = ["%dx%d-w%dx%d-%s" % (H, W, h, w, "wrap" if wr else "flat") for H, W, (h, w), _, wr in GEOS]


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


# ---- 1. the masked merge kernel --------------------------------------------------------------------------------------------

def _eps_wins(R, rows, Wn, C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((rows, Wn, C, h, w), generator=g).half() for _ in range(R)]


def _step_masks(R, H, W, seed):
    """fp32 [R, H, W] with values in {0, 0.25, 0.5, 1}; a pixel no region drew is given to region (index % R)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (R, H, W), generator=g)]
    bare = m.sum(0) == 0
    owner = (torch.arange(H * W).view(H, W) % R)
    for r in range(R):
        m[r][bare & (owner == r)] = 1.0
    return m.numpy()


def _soft_masks(R, H, W, seed):
    m = torch.rand((R, H, W), generator=torch.Generator().manual_seed(seed))
    m[0] = m[0].clamp(min=0.125)                  # every pixel is owned
    return m.numpy()


def _merge_masked(dev, es, geo, batch=None, pad=0.0, acc_fill=float("nan")):
    """All launches of a step through ops.window_merge_masked: es = R tensors [rows, Wn, C, h, w]; the windows of a region run
    as window_chunks(Wn, batch) launches whose padded slots hold `pad` and repeat the last window's offsets."""
    from lib.model_zoo import windows
    from vd_hip import ops
    H, W, h, w, wrap = geo["H"], geo["W"], geo["h"], geo["w"], geo["wrap"]
    n, R = len(geo["offs"]), len(es)
    rows, _, C = es[0].shape[:3]
    nc, m = windows.window_chunks(n, n if batch is None else batch)
    offs = np.concatenate([geo["offs"], np.repeat(geo["offs"][-1:], nc * m - n, 0)]).reshape(nc, m, 2)
    offs_d = torch.from_numpy(offs).to(dev)
    wgt, inv, masks = (torch.from_numpy(geo[k]).to(dev) for k in ("wgt", "inv_den", "masks"))
    acc = torch.full((rows, C, H, W), acc_fill, dtype=torch.float32, device=dev) if R * nc > 1 else None
    out = torch.full((rows, C, H, W), float("nan"), dtype=torch.float16, device=dev)
    for r in range(R):
        ep = torch.full((rows, nc * m, C, h, w), pad, dtype=torch.float16)
        ep[:, :n] = es[r]
        for k in range(nc):
            first, last = r == 0 and k == 0, r == R - 1 and k == nc - 1
            ret = ops.window_merge_masked(ep[:, k * m:(k + 1) * m].contiguous().to(dev), offs_d[k], wgt, masks[r], inv, H, W,
                                          min(m, n - k * m), wrap, first, last, acc=acc, out=out)
            assert ret is (out if last else acc)
            assert last or bool(torch.isnan(out).all())                  # eps is written by the last launch only
    return out.cpu()


@pytest.mark.parametrize("geo", GEOS, ids=GEO_IDS)
@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("B", [1, 3])
def test_masked_merge_uniform_is_the_restated_chain_bitwise(dev, B, C, R, geo):
    H, W, (h, w), stride, wrap = geo
    g = rc.geometry(H, W, (h, w), stride, _step_masks(R, H, W, 10 * R + B), wrap)
    es = _eps_wins(R, 2 * B, len(g["offs"]), C, h, w, 7 * B + C + R)
    out = _merge_masked(dev, es, g)
    assert out.dtype == torch.float16 and tuple(out.shape) == (2 * B, C, H, W)
    assert torch.equal(out, rc.merge_masked_restated(es, g["offs"], g["wgt"], g["masks"], g["inv_den"], H, W, wrap))


@pytest.mark.parametrize("geo", GEOS, ids=GEO_IDS)
@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("B,C", [(1, 4), (3, 3)])
def test_masked_merge_gaussian_soft_masks_within_one_fp16_rounding_of_the_exact_value(dev, B, C, R, geo):
    """|out - ref64| <= 2^-11 |ref64| + 2^-24 per element: the bound of the gaussian test of ops.window_merge."""
    H, W, (h, w), stride, wrap = geo
    g = rc.geometry(H, W, (h, w), stride, _soft_masks(R, H, W, 3 + R), wrap, weight="gaussian")
    es = _eps_wins(R, B, len(g["offs"]), C, h, w, 11 + R)
    out = _merge_masked(dev, es, g).double()
    ref = rc.merge_masked_ref64(es, g["offs"], g["wgt"], g["masks"], g["inv_den"], H, W, wrap)
    excess = (out - ref).abs() - (2.0 ** -11 * ref.abs() + 2.0 ** -24)
    print("gaussian masked merge R=%d: max |out - ref64| %.3e, max excess over the bound %.3e"
          % (R, float((out - ref).abs().max()), float(excess.max())))
    assert bool(torch.isfinite(out).all()) and float(excess.max()) <= 0.0


@pytest.mark.parametrize("geo", GEOS, ids=GEO_IDS)
@pytest.mark.parametrize("weight", ["uniform", "gaussian"])
@pytest.mark.parametrize("B,C", [(1, 3), (3, 4)])
def test_masked_merge_gives_window_merge_bits_for_ones_and_for_complementary_masks(dev, B, C, weight, geo):
    from vd_hip import ops
    H, W, (h, w), stride, wrap = geo
    g = wc.geometry(H, W, (h, w), stride, wrap, weight)
    e = _eps_wins(1, B, len(g["offs"]), C, h, w, 5)[0]
    tabs = [torch.from_numpy(g[k]).to(dev) for k in ("offs", "wgt", "inv_den")]
    ref = ops.window_merge(e.to(dev), tabs[0], tabs[1], tabs[2], H, W, len(g["offs"]), wrap, True, True).cpu()
    third = np.stack([(np.arange(W) % 3 == r)[None].repeat(H, 0) for r in range(3)]).astype(np.float32)
    for masks in (np.ones((1, H, W), dtype=np.float32), rc.half_masks(H, W), third):
        rg = rc.geometry(H, W, (h, w), stride, masks, wrap, weight)
        assert np.array_equal(rg["inv_den"], g["inv_den"])
        assert torch.equal(_merge_masked(dev, [e] * len(masks), rg), ref), len(masks)


@pytest.mark.parametrize("wrap", [False, True])
def test_nan_under_a_zero_mask_and_in_padded_slots_never_reaches_the_output(dev, wrap):
    H, W = 12, 16 if wrap else 20
    masks = rc.half_masks(H, W)
    g = rc.geometry(H, W, (8, 8), (4, 4), masks, wrap, "gaussian")
    es = _eps_wins(2, 3, len(g["offs"]), 4, 8, 8, 9)
    clean = _merge_masked(dev, es, g, batch=3, pad=0.0)
    dirty = []
    for r, e in enumerate(es):                      # NaN wherever the region's mask is 0 under the window
        e = e.clone()
        for k, (oy, ox) in enumerate(g["offs"]):
            off = torch.from_numpy(masks[r][oy:oy + 8][:, wc.cols(ox, 8, W, wrap).numpy()] == 0)
            e[:, k][..., off] = float("nan")
        assert bool(torch.isnan(e).any())
        dirty.append(e)
    out = _merge_masked(dev, dirty, g, batch=3, pad=float("nan"))
    assert bool(torch.isfinite(out).all()) and torch.equal(out, clean)


@pytest.mark.parametrize("weight", ["uniform", "gaussian"])
@pytest.mark.parametrize("wrap", [False, True])
def test_masked_merge_has_the_same_bits_however_the_launches_are_split(dev, weight, wrap):
    """Eight windows x two regions as 1, 2, 3 and 8 launches per region."""
    H, W = 12, 16 if wrap else 20
    g = rc.geometry(H, W, (8, 8), (4, 4), _soft_masks(2, H, W, 4) if weight == "gaussian" else _step_masks(2, H, W, 4), wrap, weight)
    assert len(g["offs"]) == 8
    es = _eps_wins(2, 4, 8, 3, 8, 8, 5)
    outs = [_merge_masked(dev, es, g, batch=b, pad=float("nan")) for b in (8, 4, 3, 1)]
    assert bool(torch.isfinite(outs[0]).all()) and all(torch.equal(o, outs[0]) for o in outs[1:])
    if weight == "uniform":
        assert torch.equal(outs[0], rc.merge_masked_restated(es, g["offs"], g["wgt"], g["masks"], g["inv_den"], H, W, wrap))


def test_masked_entry_point_refuses_bad_arguments(dev):
    from vd_hip import ops
    from vd_hip.loader import VdHipError, lib
    L = lib()
    f16 = dict(device=dev, dtype=torch.float16)
    win = torch.zeros((1, 2, 2, 8, 8), **f16)
    offs = torch.zeros((2, 2), device=dev, dtype=torch.int32)
    wgt, inv, mask = torch.ones((8, 8), device=dev), torch.ones((8, 12), device=dev), torch.ones((8, 12), device=dev)
    acc, eps = torch.zeros((1, 2, 8, 12), device=dev), torch.zeros((1, 2, 8, 12), **f16)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def merge(e=win, acc=acc, eps=eps, wgt=wgt, mask=mask, inv=inv, offs=offs, RB=1, C=2, H=8, W=12, h=8, w=8, slots=2, valid=2,
              wrap=0, first=1, last=1):
        return L.vd_window_merge_masked_f16(P(e), P(acc), P(eps), P(wgt), P(mask), P(inv), P(offs), RB, C, H, W, h, w, slots,
                                            valid, wrap, first, last, stream)

    assert merge() == 0 and merge(acc=None) == 0 and merge(first=1, last=0, eps=None) == 0 and merge(first=0, last=1) == 0
    bad = [dict(e=None), dict(wgt=None), dict(mask=None), dict(inv=None), dict(offs=None), dict(eps=None), dict(acc=None, last=0),
           dict(acc=None, first=0), dict(RB=0), dict(C=-2), dict(H=0), dict(W=0), dict(h=0), dict(w=0), dict(slots=0),
           dict(h=9), dict(w=13), dict(valid=0), dict(valid=3), dict(valid=-1)]
    for kw in bad:
        assert merge(**kw) < 0 and L.vd_last_error().decode().startswith("vd_window_merge_masked_f16"), kw
    assert L.vd_abi_version() == 8
    # the wrapper checks shape, dtype and device before the library is called
    M = ops.window_merge_masked
    assert M(win, offs, wgt, mask, inv, 8, 12, 2, False, True, True).shape == eps.shape
    for call in (lambda: M(win, offs, wgt, mask, inv, 8, 12, 3, False, True, True),
                 lambda: M(win, offs, wgt, mask, inv, 8, 12, 0, False, True, True),
                 lambda: M(win, offs, wgt.half(), mask, inv, 8, 12, 2, False, True, True),
                 lambda: M(win, offs, wgt, mask.half(), inv, 8, 12, 2, False, True, True),
                 lambda: M(win, offs, wgt, mask.double(), inv, 8, 12, 2, False, True, True),
                 lambda: M(win, offs, wgt, mask.cpu(), inv, 8, 12, 2, False, True, True),
                 lambda: M(win, offs, wgt, None, inv, 8, 12, 2, False, True, True),
                 lambda: M(win, offs, wgt, mask[None], inv, 8, 12, 2, False, True, True),
                 lambda: M(win, offs, wgt, mask[:, :8].contiguous(), inv, 8, 12, 2, False, True, True),
                 lambda: M(win, offs, wgt, mask.t(), inv, 8, 12, 2, False, True, True),
                 lambda: M(win, offs, wgt, mask, inv[:, :8].contiguous(), 8, 12, 2, False, True, True),
                 lambda: M(win, offs, wgt[:4].contiguous(), mask, inv, 8, 12, 2, False, True, True),
                 lambda: M(win, offs[:1], wgt, mask, inv, 8, 12, 1, False, True, True),
                 lambda: M(win, offs.long(), wgt, mask, inv, 8, 12, 2, False, True, True),
                 lambda: M(win[0], offs, wgt, mask, inv, 8, 12, 2, False, True, True),
                 lambda: M(win, offs, wgt, mask, inv, 8, 12, 2, False, False, True),
                 lambda: M(win, offs, wgt, mask, inv, 8, 12, 2, False, True, True, acc=acc.half()),
                 lambda: M(win, offs, wgt, mask, inv, 8, 12, 2, False, True, True, out=eps[:, :1]),
                 lambda: M(win.cpu(), offs, wgt, mask, inv, 8, 12, 2, False, True, True)):
        with pytest.raises(VdHipError):
            call()


# ---- 2. the regional forward -----------------------------------------------------------------------------------------------

H, W = 12, 20
SHAPE = [2, 4, H, W]
KEYS = {"window": 8, "window_stride": 4}
MASKS = rc.half_masks(H, W)


def _ci(c, u, scale, ctype="text", **kw):
    return dict({"type": ctype, "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale},
                **kw)


def _to(v, f):
    return type(v)(f(c) for c in v) if isinstance(v, (list, tuple)) else f(v)


def _on_dev(c, dev):
    f = lambda t: t.half().to(dev)
    return dict(c, conditioning=_to(c["conditioning"], f), unconditional_conditioning=f(c["unconditional_conditioning"]))


def _region_dicts(cs, R):
    """region r's sampler-style context dicts (one conditioning tensor each) of contexts whose conditioning may be a list."""
    pick = lambda c, r: c["conditioning"][r] if isinstance(c["conditioning"], (list, tuple)) else c["conditioning"]
    return [[dict(c, conditioning=pick(c, r)) for c in cs] for r in range(R)]


def _fwd_inputs(seed, B, dual):
    """x and the contexts of a forward case: regional text (A left, B right); with `dual` a global image context next to it."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, H, W), generator=g).half().float()             # fp16 values: the device sees the oracle's inputs
    r = lambda L: (torch.randn((B, L, 128), generator=g) * 0.5).half().float()
    cs = [_ci([r(77), r(77)], r(77), 7.5, ratio=0.7 if dual else 1.0)]
    if dual:
        cs.append(_ci(r(50), r(50), 7.5, "image", ratio=0.3))
    return x, cs


FWD_CASES = {"B2-guided-text": (17, 2, False, 8), "B1-guided-regional-text-global-image": (18, 1, True, 3)}


def _fwd_oracle(sd, plan, case):
    """(x, contexts, regional oracle prediction, the single-prompt windowed oracle predictions of A and of B)."""
    seed, B, dual, _ = FWD_CASES[case]
    x, cs = _fwd_inputs(seed, B, dual)
    xin, t = torch.cat([x, x]), torch.full((2 * B,), 500, dtype=torch.long)
    geo = rc.geometry(H, W, 8, 4, MASKS)
    per_region = [dc.cfg_contexts(r, True) for r in _region_dicts(cs, 2)]
    with torch.no_grad():
        ref = rc.regional_eps(sd, plan, xin, t, per_region, geo)
        single = [wc.windowed_eps(sd, plan, xin, t, ctx, geo) for ctx in per_region]
    return x, cs, ref, single


def _regional_forward(net, dev, x, cs, t, keys):
    """The sampler's own _eps, eagerly, on the canvas x: the plan, the region-major contexts and the device state as a call
    makes them."""
    from lib.model_zoo.ddim import DDIMSampler, _region_contexts, _window_args
    s = DDIMSampler(net)
    x_info = dict({"type": "image"}, **keys)
    wplan = _window_args(x_info, list(x.shape), net)
    flat = _region_contexts([_on_dev(c, dev) for c in cs], wplan, x.shape[0])
    cis, guided, _, _ = s._cfg_contexts(flat, wplan["m"])
    assert len(cis) == wplan["regions"] * len(cs)
    for ci in cis:
        ci["kv_cache"] = {}
    xd = x.half().to(dev)
    rows = (2 if guided else 1) * x.shape[0]
    ts = torch.full((rows * wplan["m"],), t, dtype=torch.long, device=dev)
    eps = s._eps(x_info, xd, ts, cis, guided, len(cs) == 1, window=s._window_state(wplan, xd, guided))
    assert eps.dtype == torch.float16 and tuple(eps.shape) == (rows,) + tuple(x.shape[1:])
    return eps.clone(), wplan


@pytest.mark.parametrize("case", list(FWD_CASES))
def test_regional_forward_vs_the_oracle_per_region_and_window(tiny, plan, dev, case):
    net, sd = tiny
    B, batch = FWD_CASES[case][1], FWD_CASES[case][3]
    x, cs, ref, single = _fwd_oracle(sd, plan, case)
    eps, wplan = _regional_forward(net, dev, x, cs, 500, dict(KEYS, window_batch=batch, region_masks=MASKS))
    assert wplan["regions"] == 2 and wplan["n"] == 8 and wplan["nc"] == -(-8 // batch)
    err = rel_l2(eps, ref)
    gaps = [rel_l2(ref[B:], e[B:]) for e in single]
    print("%s: 2 regions x %d windows as %d x %d; rel-L2 vs the regional oracle %.3e; regional vs single-prompt windowed oracle "
          "(conditional rows) %.3e (A) %.3e (B)" % (case, wplan["n"], wplan["nc"], wplan["m"], err, gaps[0], gaps[1]))
    assert min(gaps) > 2 * FWD_TOL              # the bound tells the regional prediction from either single-prompt one
    assert err < FWD_TOL


# ---- 3. loops --------------------------------------------------------------------------------------------------------------

def _case(dev, seed, shape=tuple(SHAPE)):
    """(xT, [cA, cB], u) on the device."""
    g = torch.Generator().manual_seed(seed)
    xT = torch.randn(shape, generator=g).half()
    c = [(torch.randn((shape[0], 77, 128), generator=g) * 0.5).half() for _ in range(3)]
    return xT.to(dev), [c[0].to(dev), c[1].to(dev)], c[2].to(dev)


def _make(kind, net, **kw):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from lib.model_zoo.unipc import UniPCSampler
    return {"ddim": DDIMSampler, "2m": DPMSolverSampler, "unipc": UniPCSampler, "sde": DPMSolverSDESampler}[kind](net, **kw)


def _t2i(sampler, xT, c, u, scale=7.5, steps=6, c_keys=None, **keys):
    z, _ = sampler.sample(steps=steps, shape=list(xT.shape), x_info=dict({"type": "image", "xt": xT}, **keys),
                          c_info=_ci(c, u, scale, **(c_keys or {})), verbose=False)
    return z


def _regional(sampler, xT, c, u, masks=MASKS, **keys):
    return _t2i(sampler, xT, c, u, region_masks=masks, **dict(KEYS, **keys))


# Chosen on the CPU, from the oracle loops alone: over seeds 1 .. 45 the regional and the single-prompt 6-step loops lie 0.014 ..
# 0.023 apart, and the tests below need more than 2 LATENT_TOL = 0.02 for all three solvers.  Seed 11: DDIM 0.0233 / 0.0228,
# 2M 0.0212 / 0.0209, UniPC 0.0208 / 0.0206 (against prompt A / B).
LOOP_SEED = 11


@pytest.mark.parametrize("kind", ["ddim", "2m", "unipc"])
def test_regional_loops_vs_oracle_loops(tiny, plan, dev, kind):
    net, sd = tiny
    xT, c, u = _case(dev, LOOP_SEED)
    sampler = _make(kind, net)
    z = _regional(sampler, xT, c, u)
    cpu = lambda t: t.float().cpu()
    regions = [[_ci(cpu(c[r]), cpu(u), 7.5)] for r in range(2)]
    ref = rc.oracle_loop(sd, plan, sampler, kind, cpu(xT), regions, 7.5, rc.geometry(H, W, 8, 4, MASKS))
    geo = wc.geometry(H, W, 8, 4)
    single = [wc.oracle_loop(sd, plan, sampler, kind, cpu(xT), regions[r], 7.5, geo) for r in range(2)]
    err, gaps = rel_l2(z, ref), [rel_l2(ref, s) for s in single]
    print("%s: final latent rel-L2 vs the regional oracle loop %.3e; regional vs single-prompt oracle loops %.3e (A) %.3e (B)"
          % (kind, err, gaps[0], gaps[1]))
    assert tuple(z.shape) == tuple(SHAPE) and z.dtype == xT.dtype
    assert min(gaps) > 2 * LATENT_TOL           # the bound tells the regional loop from either single-prompt loop
    assert err < LATENT_TOL


# ---- 4. bit-identities and plumbing ----------------------------------------------------------------------------------------

def test_one_region_of_ones_is_the_windowed_call_and_on_one_window_the_plain_call(tiny, dev):
    net, _ = tiny
    xT, c, u = _case(dev, 24)
    ones = np.ones((1, H, W), dtype=np.float32)
    for kind in ("ddim", "unipc"):
        z_win = _t2i(_make(kind, net), xT, c[0], u, **KEYS)
        assert torch.equal(_regional(_make(kind, net), xT, [c[0]], u, masks=ones), z_win)
        assert torch.equal(_regional(_make(kind, net), xT, c[0], u, masks=torch.from_numpy(ones)[:, None].to(dev)), z_win)
        z_plain = _t2i(_make(kind, net), xT, c[0], u)
        s = _make(kind, net)
        assert torch.equal(_t2i(s, xT, (c[0],), u, window=(H, W), region_masks=ones), z_plain)
        st = list(s._static.values())[-1]
        assert st["window"]["plan"]["key"] == (H, W, H // 2, W // 2, False, "uniform", 1, 1, 1) and st["window"]["acc"] is None
        assert not torch.equal(z_plain, z_win)
    # two regions on one window (a plain image with two prompts): not the plain call of either prompt
    z2 = _t2i(_make("ddim", net), xT, c, u, window=(H, W), region_masks=MASKS)
    assert bool(torch.isfinite(z2).all())
    assert all(rel_l2(z2, _t2i(_make("ddim", net), xT, c[r], u)) > 1e-3 for r in range(2))


@pytest.mark.parametrize("kind,batch", [("ddim", 8), ("unipc", 3)])
def test_regional_graph_replay_matches_eager_steps_and_a_fresh_sampler_bitwise(tiny, dev, monkeypatch, kind, batch):
    net, _ = tiny
    case = _case(dev, 23)
    z_graph = _regional(_make(kind, net), *case, window_batch=batch)
    assert torch.equal(_regional(_make(kind, net), *case, window_batch=batch), z_graph)
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _make(kind, net)
    assert not eager.use_graph
    assert torch.equal(z_graph, _regional(eager, *case, window_batch=batch))


def test_one_kept_graph_serves_every_mask_of_the_same_regions_and_geometry(tiny, dev):
    net, _ = tiny
    a, b = _case(dev, 25), _case(dev, 26)
    soft = np.stack([np.linspace(1.0, 0.0, W, dtype=np.float32)[None].repeat(H, 0)] * 2)
    soft[1] = 1.0 - soft[0]
    others = rc.half_masks(H, W, 7)
    fresh = {name: _regional(_make("2m", net), *case, masks=m)
             for name, case, m in (("a", a, MASKS), ("b-soft", b, soft), ("a-others", a, others))}
    off = _t2i(_make("2m", net), a[0], a[1][0], a[2], **KEYS)
    assert not torch.equal(fresh["a"], fresh["a-others"]) and not torch.equal(fresh["a"], off)
    shared = _make("2m", net)
    assert torch.equal(_regional(shared, *a), fresh["a"])
    st = list(shared._static.values())[-1]
    graph = st["graph"]
    assert graph is not None and st["window"]["plan"]["key"] == (8, 8, 4, 4, False, "uniform", 1, 8, 2)
    assert tuple(st["window"]["rmask"].shape) == (2, H, W) and tuple(st["window"]["acc"].shape) == (4, 4, H, W)
    assert len(st["c"]) == 2 and tuple(st["c"][0].shape) == (2 * 2 * 8, 77, 128)
    # other masks of the same R on the kept graph: replayed, not captured again, and a fresh sampler's bits
    assert torch.equal(_regional(shared, *b, masks=soft), fresh["b-soft"])
    assert torch.equal(_regional(shared, *a, masks=others), fresh["a-others"])
    assert len(shared._static) == 1 and list(shared._static.values())[-1]["graph"] is graph
    assert torch.equal(st["window"]["rmask"].cpu(), torch.from_numpy(others))
    # an off-call behind it gives the off bits, and the regional call after that its own again
    assert torch.equal(_t2i(shared, a[0], a[1][0], a[2], **KEYS), off) and len(shared._static) == 2
    assert torch.equal(_regional(shared, *a), fresh["a"]) and list(shared._static.values())[-1]["graph"] is graph
    shared.release_graphs()
    assert shared._static == {}


def test_regional_sde_with_seeds_repeats_and_eta_zero_is_2m(tiny, dev):
    net, _ = tiny
    xT, c, u = _case(dev, 22)
    x_info = lambda: dict({"type": "image", "xt": xT, "seeds": [5, 6], "region_masks": MASKS}, **KEYS)
    run = lambda s, **kw: s.sample(steps=6, shape=SHAPE, x_info=x_info(), c_info=_ci(c, u, 7.5), verbose=False, **kw)[0]
    shared = _make("sde", net)
    z = run(shared)
    assert bool(torch.isfinite(z).all())
    assert torch.equal(run(shared), z) and torch.equal(run(_make("sde", net)), z)
    z0 = run(_make("sde", net), eta=0.)
    assert torch.equal(z0, _regional(_make("2m", net), xT, c, u)) and not torch.equal(z0, z)


def test_regional_inpainting_returns_the_known_region_bitwise(tiny, dev):
    net, _ = tiny
    _, c, u = _case(dev, 27)
    x0 = (torch.randn(SHAPE, generator=torch.Generator().manual_seed(4)) * 0.5).half().to(dev)
    mask = torch.ones((2, 1, H, W))
    mask[..., :5, :] = 0                         # keep the top rows, across both regions
    mask = mask.half().to(dev)
    for kind in ("ddim", "2m"):
        x_info = dict({"type": "image", "x0": x0, "inpaint_mask": mask, "region_masks": MASKS}, **KEYS)
        z, _ = _make(kind, net).sample(steps=6, shape=SHAPE, x_info=x_info, c_info=_ci(c, u, 7.5, guidance_rescale=0.5),
                                       verbose=False)
        keep = (mask == 0).expand_as(x0)
        assert torch.equal(z[keep], x0[keep])
        assert rel_l2(z[~keep], x0[~keep]) > 0.1 and bool(torch.isfinite(z).all())


def test_multicontext_call_with_regional_text_and_a_global_image_context(tiny, dev):
    net, _ = tiny
    xT, c, u = _case(dev, 30)
    g = torch.Generator().manual_seed(31)
    ci, ui = [(torch.randn((2, 50, 128), generator=g) * 0.5).half().to(dev) for _ in range(2)]
    cs = lambda text: [_ci(text, u, 7.5, ratio=0.4), _ci(ci, ui, 7.5, "image", ratio=0.6)]
    run = lambda s, text, **keys: s.sample_multicontext(steps=6, shape=SHAPE, x_info=dict({"type": "image", "xt": xT}, **keys),
                                                        c_info_list=cs(text), verbose=False)[0]
    keys = dict(KEYS, region_masks=MASKS, freeu=(1.2, 1.4, 0.9, 0.2))
    shared = _make("unipc", net)
    z = run(shared, c, **keys)
    assert torch.equal(run(shared, c, **keys), z) and torch.equal(run(_make("unipc", net), c, **keys), z)
    assert bool(torch.isfinite(z).all())
    assert rel_l2(z, run(shared, c[0], **dict(KEYS, freeu=keys["freeu"]))) > 1e-3
    assert rel_l2(z, run(shared, c, **dict(KEYS, region_masks=MASKS))) > 1e-4           # FreeU acts inside each forward


def test_eager_ddim_loop_runs_regional(tiny, dev):
    """eta > 0 runs DDIM's eager loop on the same _eps: the seeded repeat and the distance from the single-prompt call."""
    net, _ = tiny
    xT, c, u = _case(dev, 29)
    outs = []
    for cond, keys in ((c, dict(KEYS, region_masks=MASKS)), (c, dict(KEYS, region_masks=MASKS)), (c[0], KEYS)):
        torch.manual_seed(3)
        outs.append(_make("ddim", net).sample(steps=6, shape=SHAPE, x_info=dict({"type": "image", "xt": xT}, **keys),
                                              c_info=_ci(cond, u, 7.5), eta=0.5, verbose=False)[0])
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())
    assert rel_l2(outs[0], outs[2]) > 1e-3


def test_sharded_world1_matches_direct_regional_sample(tiny, dev):
    from lib.model_zoo import sharded
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    gold = load_gold("ddim_tiny.npz")
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dev).half()
    ct = _ci([T(gold["c_text"]), T(gold["u_text"]).flip(1)], T(gold["u_text"]), 7.5)
    seed, steps = 3, 6
    imgs = sharded.vd_sample_sharded(net, UniPCSampler(net), steps, SHAPE, [dict(ct)], seed, guidance_scale=7.5,
                                     device_generator=True, window=8, window_stride=(4, 6), window_batch=4, region_masks=MASKS)
    torch.manual_seed(seed + 100)
    keys = {"window": 8, "window_stride": (4, 6), "window_batch": 4}
    z, _ = UniPCSampler(net).sample(steps=steps, shape=SHAPE, x_info=dict({"type": "image", "region_masks": MASKS}, **keys),
                                    c_info=dict(ct), verbose=False)
    assert torch.equal(imgs, net.vae_decode(z, which="image"))
    torch.manual_seed(seed + 100)
    z_one, _ = UniPCSampler(net).sample(steps=steps, shape=SHAPE, x_info=dict({"type": "image"}, **keys),
                                        c_info=dict(ct, conditioning=ct["conditioning"][0]), verbose=False)
    assert not torch.equal(z, z_one)
