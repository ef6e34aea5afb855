"""DeepCache sampling on the GPU: the forward in store mode (today's bits) and in reuse mode (against the fp32 restatement of
tests/deepcache_cases.py fed the oracle's own store), the work a shallow forward skips, the cuts at full width, the four samplers'
cached loops against the oracle loop with the same schedule, interval 1, graph replay against eager steps, kept graphs, and the
combinations with inpainting, the guidance rescale, seeded SDE noise and the sharding helper."""
import numpy as np
import pytest
import torch

import deepcache_cases as dc
from deepcache_cases import FWD_TOL, LATENT_TOL
from vdtest_util import full_vd_cfg, fullwidth_inputs, load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

SHAPE = [2, 4, 16, 16]


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


@pytest.fixture(scope="module")
def gold():
    return load_gold("ddim_tiny.npz")


def _inputs(seed, B, H=16, W=16, L=77, dual=False, guided=False, dim=128):
    """(x, x', [(type, context rows for the whole batch the UNet sees, ratio)]) in fp32 on the CPU, seeded."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, H, W), generator=g)
    x2 = x + 0.1 * torch.randn((B, 4, H, W), generator=g)
    rows = (2 if guided else 1) * B
    ctx = [("text", torch.randn((rows, L, dim), generator=g) * 0.5, 0.4 if dual else 1.0)]
    if dual:
        ctx.append(("image", torch.randn((rows, 50, dim), generator=g) * 0.5, 0.6))
    return x, x2, ctx


def _fwd(net, dev, x, t, ctx, guided, deep=None):
    """The product forward on x [B, ...] (handed over un-replicated with repeat = 2 when guided) at timestep t."""
    rows = (2 if guided else 1) * x.shape[0]
    x_info = {"type": "image", "x": x.half().to(dev), "repeat": 2 if guided else 1}
    if deep is not None:
        x_info["deep_cache"] = deep
    ts = torch.full((rows,), t, dtype=torch.long, device=dev)
    if len(ctx) == 1:
        return net.apply_model(x_info, ts, {"type": ctx[0][0], "c": ctx[0][1].half().to(dev)})
    return net.apply_model_multicontext(x_info, ts, [{"type": ct, "c": c.half().to(dev), "ratio": r} for ct, c, r in ctx])


def _oracle(sd, plan, x, t, ctx, guided, **kw):
    xin = torch.cat([x, x]) if guided else x
    return dc.walk(sd, plan, xin, torch.full((xin.shape[0],), t, dtype=torch.long), ctx, **kw)


# ---- 1. store mode ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("guided", [False, True])
def test_store_mode_gives_the_plain_forward_bitwise(tiny, dev, guided, dual):
    from lib.model_zoo.vd import DeepCache
    net, _ = tiny
    x, _, ctx = _inputs(11 + guided + 2 * dual, 2, dual=dual, guided=guided)
    caches = {k: DeepCache(k) for k in (1, 2, 3)}
    plain = _fwd(net, dev, x, 500, ctx, guided)
    assert all(c.buf is None for c in caches.values())           # the plain forward leaves no buffer behind
    rows = 4 if guided else 2
    shapes = {1: (rows, 16, 16, 64), 2: (rows, 16, 16, 128), 3: (rows, 8, 8, 128)}       # channels-last
    for k, cache in caches.items():
        e = _fwd(net, dev, x, 500, ctx, guided, deep=(cache, "store"))
        assert torch.equal(e, plain), k
        assert tuple(cache.buf.shape) == shapes[k] and cache.buf.dtype == torch.float16
        assert bool(torch.isfinite(cache.buf).all())
    assert torch.equal(_fwd(net, dev, x, 500, ctx, guided), plain)


# ---- 2. reuse mode with a stale store -----------------------------------------------------------------------------------

def _stale_case(net, sd, plan, dev, depth, guided, B, H=16, W=16, L=77, dual=False, dim=128):
    from lib.model_zoo.vd import DeepCache
    x, x2, ctx = _inputs(1000 * depth + 10 * B + guided + H, B, H, W, L, dual=dual, guided=guided, dim=dim)
    cache = DeepCache(depth)
    _fwd(net, dev, x, 500, ctx, guided, deep=(cache, "store"))
    e = _fwd(net, dev, x2, 450, ctx, guided, deep=(cache, "reuse"))
    ref_cache = {}
    full = _oracle(sd, plan, x, 500, ctx, guided, depth=depth, cache=ref_cache, mode="full")
    ref = _oracle(sd, plan, x2, 450, ctx, guided, depth=depth, cache=ref_cache, mode="shallow")
    assert e.shape == ((2 if guided else 1) * B, 4, H, W) and e.dtype == torch.float16
    # the kept feature itself (channels-last on the device) against the oracle's
    feat = rel_l2(cache.buf.permute(0, 3, 1, 2), ref_cache["f"])
    err = rel_l2(e, ref)
    moved = rel_l2(ref, full)
    print("depth %d guided %d B %d %dx%d: reuse rel-L2 %.3e, kept feature %.3e, shallow(x', 450) vs full(x, 500) %.3e"
          % (depth, guided, B, H, W, err, feat, moved))
    assert feat < FWD_TOL
    assert err < FWD_TOL
    assert moved > 2 * FWD_TOL           # (oracle alone, at least 0.024 over these cases) the bound tells x', t' from x, t
    return e


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_reuse_mode_with_a_stale_store_vs_restatement(tiny, plan, dev, depth, guided, B):
    net, sd = tiny
    _stale_case(net, sd, plan, dev, depth, guided, B)


@pytest.mark.parametrize("depth,guided,dual", [(1, True, False), (3, False, False), (2, True, True)])
def test_reuse_mode_on_a_non_square_latent(tiny, plan, dev, depth, guided, dual):
    """B = 3, 12 x 20 (of test_tiny_unet_ragged_shapes_vs_oracle): an odd batch and pixel counts that are no multiple of a tile."""
    net, sd = tiny
    _stale_case(net, sd, plan, dev, depth, guided, 3, 12, 20, 77, dual=dual)


def test_reuse_needs_a_matching_store(tiny, dev):
    from lib.model_zoo.vd import DeepCache
    net, _ = tiny
    x, _, ctx = _inputs(5, 2)
    cache = DeepCache(2)
    with pytest.raises(ValueError, match="store"):
        _fwd(net, dev, x, 500, ctx, False, deep=(cache, "reuse"))
    _fwd(net, dev, x, 500, ctx, False, deep=(cache, "store"))
    _fwd(net, dev, x, 500, ctx, False, deep=(cache, "reuse"))
    cache.depth = 1                              # another cut than the one the buffer was stored at
    with pytest.raises(ValueError, match="store"):
        _fwd(net, dev, x, 500, ctx, False, deep=(cache, "reuse"))
    cache.depth = 2
    x3, _, ctx3 = _inputs(6, 3)
    with pytest.raises(ValueError, match="shape"):
        _fwd(net, dev, x3, 500, ctx3, False, deep=(cache, "reuse"))
    with pytest.raises(ValueError, match="depth"):
        _fwd(net, dev, x, 500, ctx, False, deep=(DeepCache(4), "store"))


# ---- 3. work actually skipped --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("guided", [False, True])
def test_shallow_forwards_skip_library_calls(tiny, dev, guided):
    from lib.model_zoo.vd import DeepCache
    from vd_hip import ops
    net, _ = tiny
    x, _, ctx = _inputs(21, 2, guided=guided)

    def calls(deep=None):
        _fwd(net, dev, x, 500, ctx, guided, deep=deep)           # (a first forward may build weight packs)
        before = ops.LIB_CALLS[0]
        _fwd(net, dev, x, 500, ctx, guided, deep=deep)
        return ops.LIB_CALLS[0] - before

    full = calls()
    store, reuse = {}, {}
    for k in (1, 2, 3):
        cache = DeepCache(k)
        store[k] = calls((cache, "store"))
        reuse[k] = calls((cache, "reuse"))
    print("library calls per forward: full %d, store %r, reuse %r" % (full, store, reuse))
    assert all(store[k] == full for k in store)
    assert 0 < reuse[1] < reuse[2] < reuse[3] < full


# ---- 4. full width -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def full(dev):
    from lib.model_zoo import get_model
    net = get_model()(full_vd_cfg(with_vae=False), verbose=False)
    sd = synth_into(net, 7)
    net = net.half()
    net.to(dev)
    return net, sd


@pytest.mark.parametrize("depth,guided", [(1, True), (4, False)])
def test_full_width_store_and_reuse_vs_restatement(full, dev, depth, guided):
    """B = 2 at 16 x 16.  Depth 1 guided: no context block in front of the cut, so the skips are replicated at the jump, at width
    320 where the CFG head share applies to the full forward.  Depth 4 unguided: the prefix crosses a Downsample and the suffix
    resumes in front of an Upsample ([B, 8, 8, 640] kept)."""
    from lib.model_zoo.vd import DeepCache
    from oracle import vd_oracle as O
    net, sd = full
    plan = O.unet_plan()
    inp = fullwidth_inputs()
    x = inp["x"].float()
    x2 = x + 0.1 * torch.randn(x.shape, generator=torch.Generator().manual_seed(17))
    ctx = [("text", (torch.cat([inp["ut"], inp["ct"]]) if guided else inp["ct"]).float(), 1.0)]
    cache = DeepCache(depth)
    plain = _fwd(net, dev, x, 500, ctx, guided)
    e_store = _fwd(net, dev, x, 500, ctx, guided, deep=(cache, "store"))
    assert torch.equal(e_store, plain)
    rows = 4 if guided else 2
    assert tuple(cache.buf.shape) == {1: (rows, 16, 16, 320), 4: (rows, 8, 8, 640)}[depth]
    e = _fwd(net, dev, x2, 450, ctx, guided, deep=(cache, "reuse"))
    ref_cache = {}
    ref_full = _oracle(sd, plan, x, 500, ctx, guided, depth=depth, cache=ref_cache, mode="full")
    ref = _oracle(sd, plan, x2, 450, ctx, guided, depth=depth, cache=ref_cache, mode="shallow")
    errs = (rel_l2(e_store, ref_full), rel_l2(cache.buf.permute(0, 3, 1, 2), ref_cache["f"]), rel_l2(e, ref))
    print("full width depth %d guided %d: store %.3e, kept feature %.3e, reuse %.3e" % ((depth, guided) + errs))
    assert all(v < FWD_TOL for v in errs)


# ---- 5. loops ----------------------------------------------------------------------------------------------------------

def _ci(c, u, scale, ctype="text", **kw):
    return dict({"type": ctype, "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale},
                **kw)


def _on_dev(c, dev):
    return dict(c, conditioning=c["conditioning"].half().to(dev),
                unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))


def _make(kind, net):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    from lib.model_zoo.unipc import UniPCSampler
    return {"ddim": DDIMSampler, "2m": DPMSolverSampler, "unipc": UniPCSampler}[kind](net)


@pytest.mark.parametrize("kind,steps,N,depth,dual", [("ddim", 6, 2, 1, False), ("ddim", 9, 3, 2, False), ("2m", 10, 2, 1, False),
                                                     ("unipc", 10, 2, 1, False), ("2m", 8, 3, 3, True)])
def test_cached_loops_vs_oracle_loop_with_the_same_schedule(tiny, plan, dev, gold, kind, steps, N, depth, dual):
    """`steps` is what sample() is asked for; the uniform grid of 6 steps holds 7 timesteps, so that call runs 7.  There is no
    uniform grid of 9 steps (it would hold timestep 1000, and DDIM's own parameters raise, as the reference's do): the 9-step
    case is the 10-step grid entered at its ninth timestep (x0 + x0_forward_timesteps = 9 with injected forward noise), which
    runs exactly 9 steps, numbered 0 .. 8 from the first one the call runs."""
    net, sd = tiny
    xT = torch.from_numpy(gold["xT"]).float()
    start = {"xt": xT.half().to(dev)}
    if steps == 9:
        from oracle import vd_oracle as O
        x0, noise = torch.from_numpy(gold["x0"]).float(), torch.from_numpy(gold["q_noise"]).float()
        start = {"x0": x0.half().to(dev), "x0_forward_timesteps": 9, "x0_noise": noise.half().to(dev)}
        a = float(np.float32(O.register_schedule()["alphas_cumprod"].numpy()[901]))      # the tenth timestep of the 10-step grid
        xT = np.sqrt(a) * x0.half().float() + np.sqrt(1 - a) * noise.half().float()
    cs = [_ci(torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"]), 7.5)]
    if dual:
        cs = [dict(cs[0], ratio=0.4), _ci(torch.from_numpy(gold["c_img"]), torch.from_numpy(gold["u_img"]), 7.5, "image", ratio=0.6)]
    sampler = _make(kind, net)
    x_info = lambda **kw: dict({"type": "image"}, **start, **kw)
    grid = 10 if steps == 9 else steps

    def run(**kw):
        if dual:
            return sampler.sample_multicontext(steps=grid, shape=SHAPE, x_info=x_info(**kw),
                                               c_info_list=[_on_dev(c, dev) for c in cs], verbose=False)
        return sampler.sample(steps=grid, shape=SHAPE, x_info=x_info(**kw), c_info=_on_dev(cs[0], dev), verbose=False)

    z, inter = run(cache_interval=N, cache_depth=depth)
    if steps == 9:
        assert int(sampler.ddim_timesteps[9]) == 901
        sampler.ddim_timesteps = sampler.ddim_timesteps[:9]          # the loop the call walked
    total = len(sampler.ddim_timesteps)
    assert total == {6: 7}.get(steps, steps)
    assert inter["cache_full_steps"] == list(range(0, total, N)) == dc.full_steps(total, N)
    ref = dc.oracle_loop(sd, plan, sampler, kind, xT, cs, 7.5, interval=N, depth=depth)
    plain = dc.oracle_loop(sd, plan, sampler, kind, xT, cs, 7.5)
    z_plain, i_plain = run()
    if steps == 9:
        sampler.ddim_timesteps = sampler.ddim_timesteps[:9]
    assert "cache_full_steps" not in i_plain
    err, gap = rel_l2(z, ref), rel_l2(ref, plain)
    print("%s %d steps N %d depth %d dual %d: rel-L2 vs the cached oracle loop %.3e; cached vs uncached oracle loop %.3e; "
          "uncached product vs uncached oracle %.3e" % (kind, steps, N, depth, dual, err, gap, rel_l2(z_plain, plain)))
    assert err < LATENT_TOL
    assert rel_l2(z_plain, plain) < LATENT_TOL
    # the two oracle loops are closer to each other (6e-3 .. 7e-3 on these cases) than the bound is wide, so the bound alone would
    # pass a loop that ignores the keys: the cached product loop must also be nearer to the cached oracle loop than to the other
    assert err < rel_l2(z, plain) and rel_l2(z_plain, plain) < rel_l2(z_plain, ref)


# ---- 6. - 8. interval 1, graphs ---------------------------------------------------------------------------------------------

def _case(dev, seed, shape=tuple(SHAPE)):
    g = torch.Generator().manual_seed(seed)
    xT = torch.randn(shape, generator=g).half().to(dev)
    c = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half().to(dev)
    u = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half().to(dev)
    return xT, c, u


def _t2i(sampler, xT, c, u, scale, steps, **keys):
    z, _ = sampler.sample(steps=steps, shape=list(xT.shape), x_info=dict({"type": "image", "xt": xT}, **keys),
                          c_info=_ci(c, u, scale), verbose=False)
    return z


def test_interval_one_is_the_uncached_call(tiny, dev):
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    case = _case(dev, 31)
    sampler = DDIMSampler(net)
    z = _t2i(sampler, *case, 7.5, 6)
    z1 = _t2i(sampler, *case, 7.5, 6, cache_interval=1)
    z2 = _t2i(sampler, *case, 7.5, 6, cache_interval=1, cache_depth=3)
    assert torch.equal(z1, z) and torch.equal(z2, z)
    assert len(sampler._static) == 1
    st = next(iter(sampler._static.values()))
    assert "deep" not in st and "graph_shallow" not in st
    assert torch.equal(_t2i(DDIMSampler(net), *case, 7.5, 6, cache_interval=1), z)


@pytest.mark.parametrize("kind", ["ddim", "unipc"])
def test_cached_graph_replay_matches_eager_bitwise(tiny, dev, monkeypatch, kind):
    net, _ = tiny
    case = _case(dev, 5)
    z_graph = _t2i(_make(kind, net), *case, 7.5, 8, cache_interval=3, cache_depth=2)
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _make(kind, net)
    assert not eager.use_graph
    assert torch.equal(z_graph, _t2i(eager, *case, 7.5, 8, cache_interval=3, cache_depth=2))


def test_kept_graphs_serve_every_interval_and_leave_uncached_calls_alone(tiny, dev):
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    net, _ = tiny
    shared = DPMSolverSampler(net)
    a, b = _case(dev, 6), _case(dev, 7)
    z_plain = _t2i(shared, *a, 7.5, 6)                                   # before any cached call
    z_a = _t2i(shared, *a, 7.5, 6, cache_interval=2)
    cached = [st for st in shared._static.values() if "deep" in st]
    assert len(cached) == 1 and len(shared._static) == 2
    st = cached[0]
    graphs = (st["graph"], st["graph_shallow"])
    assert all(g is not None for g in graphs) and graphs[0] is not graphs[1]
    buf = st["deep"].buf
    assert buf is not None and tuple(buf.shape) == (4, 16, 16, 64)
    assert torch.equal(_t2i(shared, *a, 7.5, 6), z_plain)                # an uncached call in between
    z_b = _t2i(shared, *b, 3.0, 10, cache_interval=3)
    assert len(shared._static) == 2
    assert (st["graph"], st["graph_shallow"]) == graphs and st["deep"].buf is buf        # replayed, not captured again
    assert torch.equal(z_b, _t2i(DPMSolverSampler(net), *b, 3.0, 10, cache_interval=3))
    assert torch.equal(z_a, _t2i(DPMSolverSampler(net), *a, 7.5, 6, cache_interval=2))
    assert torch.equal(_t2i(shared, *a, 7.5, 6), z_plain)
    assert rel_l2(z_a, z_plain) > 1e-4                                   # the cached call is another computation
    # another depth is another pair of graphs
    _t2i(shared, *a, 7.5, 6, cache_interval=2, cache_depth=2)
    newest = list(shared._static.values())[-1]
    assert newest is not st and newest["deep"].depth == 2 and newest["graph_shallow"] is not None
    shared.release_graphs()
    assert shared._static == {}


# ---- 9. combinations -------------------------------------------------------------------------------------------------------

def test_cached_inpainting_with_rescale_returns_the_known_region_bitwise(tiny, dev):
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    net, _ = tiny
    _, c, u = _case(dev, 9)
    x0 = (torch.randn(SHAPE, generator=torch.Generator().manual_seed(4)) * 0.5).half().to(dev)
    mask = torch.ones((2, 1, 16, 16))
    mask[..., :6, :] = 0                         # keep the top rows
    mask = mask.half().to(dev)
    z, inter = DPMSolverSampler(net).sample(steps=6, shape=SHAPE,
                                            x_info={"type": "image", "x0": x0, "inpaint_mask": mask, "cache_interval": 2},
                                            c_info=_ci(c, u, 7.5, guidance_rescale=0.7), verbose=False)
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(z[keep], x0[keep])
    assert rel_l2(z[~keep], x0[~keep]) > 0.1 and bool(torch.isfinite(z).all())
    assert inter["cache_full_steps"] == [0, 2, 4, 6] and len(inter["guidance_rescale"]) == 2     # (the 6-step grid: 7 timesteps)


def test_cached_sde_call_with_seeds_repeats_bitwise(tiny, dev):
    from lib.model_zoo.dpm_solver import DPMSolverSDESampler
    net, _ = tiny
    _, c, u = _case(dev, 12)
    run = lambda s, **kw: s.sample(steps=8, shape=SHAPE, x_info=dict({"type": "image", "seeds": [5, 6]}, **kw),
                                   c_info=_ci(c, u, 7.5), verbose=False)[0]
    shared = DPMSolverSDESampler(net)
    z = run(shared, cache_interval=2)
    assert bool(torch.isfinite(z).all())
    assert torch.equal(run(shared, cache_interval=2), z)                 # on the kept graphs
    assert torch.equal(run(DPMSolverSDESampler(net), cache_interval=2), z)
    assert not torch.equal(run(shared), z)


def test_eager_ddim_loop_follows_the_schedule(tiny, plan, dev, gold):
    """eta > 0 runs DDIM's eager loop, which hands the mode of each step to the forward like the static loop: seeded, the cached
    call repeats bit for bit, lists the static loop's schedule and differs from the uncached call on the same noise."""
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    xT, c, u = _case(dev, 14)
    outs = []
    for _ in range(2):
        torch.manual_seed(3)
        z, inter = DDIMSampler(net).sample(steps=6, shape=SHAPE, x_info={"type": "image", "xt": xT, "cache_interval": 2},
                                           c_info=_ci(c, u, 7.5), eta=0.5, verbose=False)
        assert inter["cache_full_steps"] == [0, 2, 4, 6] and bool(torch.isfinite(z).all())
        outs.append(z)
    assert torch.equal(outs[0], outs[1])
    torch.manual_seed(3)
    z_plain, _ = DDIMSampler(net).sample(steps=6, shape=SHAPE, x_info={"type": "image", "xt": xT}, c_info=_ci(c, u, 7.5), eta=0.5,
                                         verbose=False)
    assert rel_l2(outs[0], z_plain) > 1e-4


def test_sharded_world1_matches_direct_cached_sample(tiny, dev, gold):
    from lib.model_zoo import sharded
    from lib.model_zoo.unipc import UniPCSampler
    net, _ = tiny
    T = lambda a: torch.from_numpy(np.asarray(a)).to(dev).half()
    ct = _ci(T(gold["c_text"]), T(gold["u_text"]), 7.5)
    seed, steps = 3, 6
    imgs = sharded.vd_sample_sharded(net, UniPCSampler(net), steps, SHAPE, [dict(ct)], seed, guidance_scale=7.5,
                                     device_generator=True, cache_interval=2, cache_depth=2)
    torch.manual_seed(seed + 100)
    z, _ = UniPCSampler(net).sample(steps=steps, shape=SHAPE, x_info={"type": "image", "cache_interval": 2, "cache_depth": 2},
                                    c_info=dict(ct), verbose=False)
    assert torch.equal(imgs, net.vae_decode(z, which="image"))
    torch.manual_seed(seed + 100)
    z_plain, _ = UniPCSampler(net).sample(steps=steps, shape=SHAPE, x_info={"type": "image"}, c_info=dict(ct), verbose=False)
    assert not torch.equal(z, z_plain)
