"""HyperTile on the GPU: the two copies (vd_tile_tokens_f16, vd_untile_tokens_f16 through vd_hip.ops) bit for bit against
reshape / permute, the locality a tiled CrossAttention must show, its composition from the library's own attention, one
SpatialTransformer at the full widths, the tiny model's forward and the four samplers' loops against the fp32 restatement of
tests/hypertile_cases.py, and the bit identities of the sampler keys (off = today's bits; graph replay = eager steps = a fresh
sampler)."""
import ctypes

import pytest
import torch

import hypertile_cases as hc
from hypertile_cases import FWD_TOL, LATENT_TOL
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

SHAPE = [2, 4, 16, 16]
SENTINEL = -21846          # 0xAAAA as int16: a NaN-free fp16 pattern (-0.0520) no test input holds in every chunk


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


def _seeded(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.dim() >= 2:
                v = torch.randn(p.shape, generator=g) * (p[0].numel() ** -0.5)
            elif n.endswith("weight"):
                v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
            else:
                v = 0.1 * torch.randn(p.shape, generator=g)
            p.copy_(v.half().float())
    return g


# ---- 1. the two copies -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,th,tw,cols", hc.KERNEL_CASES)
def test_tile_and_untile_are_the_permutation_bit_for_bit(dev, B, H, W, th, tw, cols):
    from vd_hip import loader, ops
    x = hc.kernel_input(B, H, W, cols, 10 * H + W)
    ref = hc.tile_ref(x, H, W, th, tw)
    xd = x.to(dev)
    t = ops.tile_tokens(xd, H, W, th, tw)
    nt = (H // th) * (W // tw)
    assert t.is_contiguous() and tuple(t.shape) == (B * nt, th * tw, cols) and torch.equal(t.cpu(), ref)
    if nt == 1:
        assert torch.equal(t.view(B, H * W, cols), xd)                  # one tile: the identity
    assert torch.equal(ops.untile_tokens(t, B, H, W, th, tw), xd)       # the round trip
    # tile into a buffer pre-filled with a sentinel, two rows longer than the result: every row is written, none behind the end
    buf = torch.full((B * H * W + 2, cols), SENTINEL, dtype=torch.int16, device=dev)
    rc = loader.lib().vd_tile_tokens_f16(ctypes.c_void_p(xd.data_ptr()), cols, H * W * cols, cols, B, H, W, th, tw,
                                         ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert torch.equal(buf[:B * H * W].view(torch.float16).cpu(), ref.reshape(B * H * W, cols)) and bool((buf[B * H * W:] == SENTINEL).all())
    # untile into a strided view of a sentinel buffer: the columns beside the view and the sample in front keep the sentinel
    wide = torch.full((B + 1, H * W, cols + 16), SENTINEL, dtype=torch.int16, device=dev).view(torch.float16)
    out = ops.untile_tokens(t, B, H, W, th, tw, out=wide[1:, :, 8:8 + cols])
    assert out.data_ptr() == wide[1:, :, 8:8 + cols].data_ptr() and torch.equal(wide[1:, :, 8:8 + cols], xd)
    keep = wide.view(torch.int16)
    assert bool((keep[0] == SENTINEL).all()) and bool((keep[1:, :, :8] == SENTINEL).all()) and bool((keep[1:, :, 8 + cols:] == SENTINEL).all())
    # every row exactly once: the inputs' chunks are all distinct, so the multiset of rows is the input's
    assert torch.equal(torch.sort(t.cpu().view(-1, cols)[:, 0].float() + 2048 * t.cpu().view(-1, cols)[:, 1].float())[0],
                       torch.sort(x.view(-1, cols)[:, 0].float() + 2048 * x.view(-1, cols)[:, 1].float())[0])


@pytest.mark.parametrize("B,H,W,th,tw,c", [(2, 8, 8, 4, 4, 24), (3, 4, 12, 2, 3, 320)])
def test_strided_sources_the_slices_of_a_fused_qkv(dev, B, H, W, th, tw, c):
    from vd_hip import ops
    qkv = hc.kernel_input(B + 1, H, W, 3 * c, 77).to(dev)
    for s in range(3):                                       # q, k, v: ldx = 3 c, the k and v slices start inside a row
        part = qkv[..., s * c:(s + 1) * c]
        t = ops.tile_tokens(part, H, W, th, tw)
        assert torch.equal(t, hc.tile_ref(part, H, W, th, tw)) and torch.equal(ops.untile_tokens(t, B + 1, H, W, th, tw), part)
    view = qkv[1:]                                           # a batch slice of the fused tensor
    t = ops.tile_tokens(view, H, W, th, tw)
    assert torch.equal(t, hc.tile_ref(view, H, W, th, tw))
    assert torch.equal(t[..., c:2 * c], ops.tile_tokens(view[..., c:2 * c], H, W, th, tw))


def test_entries_refuse_bad_arguments_and_launch_nothing(dev):
    from vd_hip import ops
    z = lambda *shape: torch.zeros(shape, dtype=torch.float16, device=dev)
    calls = ops.LIB_CALLS[0]
    with pytest.raises(ops.VdHipError, match="vd_tile_tokens_f16.*multiple of 8"):
        ops.tile_tokens(z(1, 16, 12), 4, 4, 2, 2)
    with pytest.raises(ops.VdHipError, match="vd_tile_tokens_f16.*divide"):
        ops.tile_tokens(z(1, 16, 8), 4, 4, 3, 2)
    with pytest.raises(ops.VdHipError, match="vd_tile_tokens_f16.*divide"):
        ops.tile_tokens(z(1, 24, 8), 4, 6, 2, 4)
    with pytest.raises(ops.VdHipError, match="vd_tile_tokens_f16.*aligned"):
        ops.tile_tokens(z(1, 16, 16)[..., 4:12], 4, 4, 2, 2)             # rows start 8 bytes off
    with pytest.raises(ops.VdHipError, match="vd_tile_tokens_f16.*aligned"):
        ops.tile_tokens(z(1, 16, 20)[..., :8], 4, 4, 2, 2)               # ldx = 20
    with pytest.raises(ops.VdHipError, match="vd_untile_tokens_f16.*aligned"):
        ops.untile_tokens(z(4, 4, 8), 1, 4, 4, 2, 2, out=z(1, 16, 16)[..., 4:12])
    assert ops.LIB_CALLS[0] == calls + 6                     # each reached the library, which refused in front of the launch
    for bad in (lambda: ops.tile_tokens(z(1, 16, 8), 4, 5, 2, 1), lambda: ops.tile_tokens(z(1, 16, 8), 4, 4, 0, 2),
                lambda: ops.tile_tokens(z(1, 16, 8), 4, 4, 2.0, 2), lambda: ops.tile_tokens(z(16, 8), 4, 4, 2, 2),
                lambda: ops.tile_tokens(z(1, 16, 8).float(), 4, 4, 2, 2), lambda: ops.tile_tokens(z(1, 16, 8).cpu(), 4, 4, 2, 2)):
        with pytest.raises(ops.VdHipError, match="tile_tokens|x must"):
            bad()
    for bad in (lambda: ops.untile_tokens(z(4, 4, 8), 2, 4, 4, 2, 2), lambda: ops.untile_tokens(z(4, 3, 8), 1, 4, 4, 2, 2),
                lambda: ops.untile_tokens(z(4, 4, 8), 1, 4, 4, 2, 2, out=z(1, 16, 16))):
        with pytest.raises(ops.VdHipError, match="untile_tokens"):
            bad()
    assert ops.LIB_CALLS[0] == calls + 6
    torch.cuda.synchronize()


# ---- 2. locality and composition -------------------------------------------------------------------------------------------------

def _attn(dev, C, seed):
    from lib.model_zoo.attention import CrossAttention
    heads = 8
    attn = CrossAttention(C, heads=heads, dim_head=C // heads)
    g = _seeded(attn, seed)
    return attn.half().to(dev), g


def test_a_tile_sees_only_itself(dev):
    """Fails without the feature: width 320, a 16 x 16 grid, tile 8.  New input rows in tile (0, 0) leave the output rows of the
    other three tiles bit-identical; in the untiled attention the same change reaches them."""
    attn, g = _attn(dev, 320, 1)
    H = W = 16
    x = torch.randn((2, H * W, 320), generator=g).half()
    y = x.clone()
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[:8, :8] = True
    inside = inside.flatten()
    y[:, inside] = torch.randn((2, 64, 320), generator=g).half()
    xd, yd = x.to(dev), y.to(dev)
    tx, ty = attn(xd, tile=(H, W, 8, 8)), attn(yd, tile=(H, W, 8, 8))
    assert tuple(tx.shape) == (2, H * W, 320)
    assert torch.equal(tx[:, ~inside], ty[:, ~inside]) and not torch.equal(tx[:, inside], ty[:, inside])
    px, py = attn(xd), attn(yd)
    changed = (px[:, ~inside] != py[:, ~inside]).any(-1)
    assert bool(changed.all())                               # untiled: every other row moved
    assert not torch.equal(tx, px)
    # one tile is the untiled attention, bit for bit
    assert torch.equal(attn(xd, tile=(H, W, 16, 16)), px)


@pytest.mark.parametrize("C,H,W,th,tw", [(320, 16, 16, 8, 8), (640, 8, 12, 4, 6)])
def test_tiled_attention_is_the_librarys_attention_on_the_permuted_qkv(dev, C, H, W, th, tw):
    from vd_hip import ops
    attn, g = _attn(dev, C, C)
    c = attn.inner
    x = torch.randn((3, H * W, C), generator=g).half().to(dev)
    res = torch.randn((3, H * W, C), generator=g).half().to(dev)
    out = attn(x, res=res, tile=(H, W, th, tw))
    qkv = ops.linear(x, attn._w_qkv())
    m = hc.tile_ref(qkv, H, W, th, tw).contiguous()
    a = ops.attention(m[..., :c], m[..., c:2 * c], m[..., 2 * c:], attn.heads, scale=attn.scale)
    a = hc.untile_ref(a, 3, H, W, th, tw).contiguous()
    assert torch.equal(out, attn.to_out[0](a, res=res))
    assert torch.equal(attn(x, res=res, qkv=qkv, tile=(H, W, th, tw)), out)       # q | k | v handed in by the caller
    # identity rows (perturbed-attention guidance) are per token: samples >= ident_from are to_out(v), the others the tiled bits
    pert = attn(x, res=res, tile=(H, W, th, tw), ident_from=1)
    assert torch.equal(pert[:1], out[:1]) and torch.equal(pert[1:], attn(x, res=res, ident_from=1)[1:])


def test_refusals_of_the_attention_layer(dev):
    from vd_hip import ops
    attn, g = _attn(dev, 320, 3)
    x = torch.zeros((1, 64, 320), dtype=torch.float16, device=dev)
    ctx = torch.zeros((1, 7, 320), dtype=torch.float16, device=dev)
    with pytest.raises(ops.VdHipError, match="tile.*self-attention"):
        attn(x, context=ctx, tile=(8, 8, 4, 4))
    with pytest.raises(ops.VdHipError, match="tile.*self-attention"):
        attn(x, kv=torch.zeros((1, 7, 640), dtype=torch.float16, device=dev), tile=(8, 8, 4, 4))
    with pytest.raises(ops.VdHipError, match="tile.*tome"):
        attn(x, tile=(8, 8, 4, 4), tome=(8, 8, 16, x))
    with pytest.raises(ops.VdHipError, match="tile.*sag"):
        attn(x, tile=(8, 8, 4, 4), sag=torch.zeros((1, 64), dtype=torch.float32, device=dev))
    for bad in ((8, 4, 4, 4), (8, 8, 3, 4), (8, 8, 4, 0), (4, 16, 4, 3)):
        with pytest.raises(ops.VdHipError, match="tile"):
            attn(x, tile=bad)


def _block(dev, C, seed):
    from lib.model_zoo.attention import SpatialTransformer
    heads = 8
    st = SpatialTransformer(C, heads, C // heads, context_dim=768)
    g = _seeded(st, seed)
    sd = {"b." + k: v.detach().clone().float() for k, v in st.state_dict().items()}
    return st.half().to(dev), sd, g, heads


def test_block_under_repeat_2_tiles_once_per_pair_and_composes(dev, monkeypatch):
    """Width 320 with the shared CFG head: the tiled self-attention runs on ONE replica, and the block with the two HIP copies
    replaced by torch's reshape / permute gives the same bits."""
    from vd_hip import ops
    st, _, g, _ = _block(dev, 320, 11)
    assert st.shares_cfg_head()
    B, side = 2, 16
    xd = torch.randn((B, side, side, 320), generator=g).half().to(dev)
    ctx = (torch.randn((2 * B, 77, 768), generator=g) * 0.5).half().to(dev)
    seen = []
    real_tile, real_untile = ops.tile_tokens, ops.untile_tokens
    monkeypatch.setattr(ops, "tile_tokens", lambda x, *a: seen.append(tuple(x.shape)) or real_tile(x, *a))
    out = st(xd, ctx, tile=(8, 8), repeat=2)
    assert seen == [(B, side * side, 960)] and tuple(out.shape) == (2 * B, side, side, 320)
    monkeypatch.setattr(ops, "tile_tokens", lambda x, H, W, th, tw: hc.tile_ref(x, H, W, th, tw).contiguous())
    monkeypatch.setattr(ops, "untile_tokens", lambda a, B_, H, W, th, tw: hc.untile_ref(a, B_, H, W, th, tw).contiguous())
    assert torch.equal(st(xd, ctx, tile=(8, 8), repeat=2), out)
    monkeypatch.setattr(ops, "tile_tokens", real_tile)
    monkeypatch.setattr(ops, "untile_tokens", real_untile)
    assert not torch.equal(st(xd, ctx, repeat=2), out)


# ---- 3. one block at the full widths ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,side,tile,repeat", [(320, 16, 8, 2), (640, 8, 4, 1), (1280, 8, 4, 1)])
def test_one_block_at_the_full_widths_vs_the_fp32_restatement(dev, C, side, tile, repeat):
    """One SpatialTransformer at each full width -- 320: q | k | v from the chained entry kernel, the self-attention once per
    guidance pair (repeat = 2); 640 / 1280: the block's own fused projection -- with seeded weights (proj_out not left at zero),
    against the block of tests/hypertile_cases.py.  Compared on what the block adds to its input (out - x), sample by sample, with
    the project's forward bound; the tiled block must sit further than that bound from the untiled one."""
    from oracle import vd_oracle as O
    st, sd, g, heads = _block(dev, C, C)
    B = 2
    x = torch.randn((B, C, side, side), generator=g).half().float()
    ctx = (torch.randn((repeat * B, 77, 768), generator=g) * 0.5).half().float()
    xd = x.permute(0, 2, 3, 1).contiguous().half().to(dev)
    kw = {"repeat": repeat} if repeat > 1 else {}
    out = st(xd, ctx.half().to(dev), tile=(tile, tile), **kw)
    xr = torch.cat([x] * repeat)
    with torch.no_grad():
        ref = hc.spatial_transformer(sd, "b", xr, ctx, heads, tile, tile) - xr
        off = O.spatial_transformer(sd, "b", xr, ctx, heads) - xr
    delta = (out.float() - torch.cat([xd] * repeat).float()).permute(0, 3, 1, 2).cpu()
    errs = [rel_l2(delta[b], ref[b]) for b in range(repeat * B)]
    plain = (st(xd, ctx.half().to(dev), **kw).float() - torch.cat([xd] * repeat).float()).permute(0, 3, 1, 2).cpu()
    print("width %d: block delta vs the fp32 tiled block per sample %s; plain block vs the untiled oracle %.3e; tiled vs untiled on "
          "the device %.3e" % (C, ["%.3e" % e for e in errs], rel_l2(plain, off), rel_l2(delta, plain)))
    assert all(e < FWD_TOL for e in errs)
    assert rel_l2(plain, off) < FWD_TOL and rel_l2(delta, plain) > FWD_TOL
    assert torch.equal(st(xd, ctx.half().to(dev), tile=(tile, tile), **kw), out)          # the same call twice: the same bits


# ---- 4. the tiny model's forward -------------------------------------------------------------------------------------------------

def _inputs(seed, B, dual, guided):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, 16, 16), generator=g).half().float()
    rows = lambda L: (torch.randn(((2 if guided else 1) * B, L, 128), generator=g) * 0.5).half().float()
    ctx = [("text", rows(77), 0.4 if dual else 1.0)]
    if dual:
        ctx.append(("image", rows(50), 0.6))
    return x, ctx


def _fwd(net, dev, x, t, ctx, reps, **keys):
    x_info = dict({"type": "image", "x": x.half().to(dev), "repeat": reps}, **keys)
    ts = torch.full((reps * x.shape[0],), t, dtype=torch.long, device=dev)
    if len(ctx) == 1:
        return net.apply_model(x_info, ts, {"type": ctx[0][0], "c": ctx[0][1].half().to(dev)})
    return net.apply_model_multicontext(x_info, ts, [{"type": ct, "c": c.half().to(dev), "ratio": r} for ct, c, r in ctx])


@pytest.mark.parametrize("dual,guided,tile,md", [(False, True, 4, 2), (True, True, 8, 1), (False, False, 8, 1), (True, False, 4, 2)])
def test_forward_vs_the_fp32_walk(tiny, plan, dev, dual, guided, tile, md):
    from lib.model_zoo.vd import HyperTile
    net, sd = tiny
    B, reps = 2, 2 if guided else 1
    x, ctx = _inputs(31 + dual + 2 * guided, B, dual, guided)
    ht = HyperTile(tile, md)
    e = _fwd(net, dev, x, 500, ctx, reps, hypertile=ht)
    xin = torch.cat([x] * reps)
    t = torch.full((xin.shape[0],), 500, dtype=torch.long)
    tiles = []
    ref = hc.walk(sd, plan, xin, t, ctx, tile, md, tiles=tiles)
    assert tiles == ([(256, 4)] * 3 if md == 1 else [(256, 16), (64, 4), (64, 4), (64, 4), (64, 4), (256, 16), (256, 16)])
    plain = _fwd(net, dev, x, 500, ctx, reps)
    err, moved = rel_l2(e, ref), rel_l2(e, plain)
    print("dual %d guided %d tile %d max_downsample %d: forward vs the fp32 walk %.3e; tiled vs untiled forward %.3e; untiled vs its walk "
          "%.3e" % (dual, guided, tile, md, err, moved, rel_l2(plain, hc.walk(sd, plan, xin, t, ctx))))
    assert err < FWD_TOL and moved > FWD_TOL
    # off: absent, None and 0 are today's forward, bit for bit; the int key is the ready object
    assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, hypertile=None), plain)
    assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, hypertile=0, hypertile_max_downsample=md), plain)
    assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, hypertile=tile, hypertile_max_downsample=md), e)
    assert torch.equal(_fwd(net, dev, x, 500, ctx, reps, hypertile=16, hypertile_max_downsample=4), plain)       # every level fits one tile


# ---- 5. loops --------------------------------------------------------------------------------------------------------------------

def _ci(c, u, scale, ctype="text", **kw):
    return dict({"type": ctype, "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale}, **kw)


def _on_dev(c, dev):
    return dict(c, conditioning=c["conditioning"].half().to(dev), unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))


def _make(kind, net, **kw):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    from lib.model_zoo.unipc import UniPCSampler
    return {"ddim": DDIMSampler, "2m": DPMSolverSampler, "unipc": UniPCSampler, "sde": DPMSolverSDESampler}[kind](net, **kw)


def _gold_case(gold, scale=7.5):
    xT = torch.from_numpy(gold["xT"]).float()
    return xT, [_ci(torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"]), scale)]


def _sample(sampler, dev, xT, cs, steps=6, c_keys=None, call=None, **keys):
    """steps = 6: the uniform schedule's spacing 1000 // 6 = 166 gives the SEVEN timesteps 1, 167, ..., 997."""
    x_info = dict({"type": "image", "xt": xT.half().to(dev)}, **keys)
    c = dict(_on_dev(cs[0], dev), **(c_keys or {}))
    return sampler.sample(steps=steps, shape=list(xT.shape), x_info=x_info, c_info=c, verbose=False, **(call or {}))


TILES_TINY = {(8, 1): [(256, 4)] * 3, (4, 1): [(256, 16)] * 3,
              (4, 2): [(256, 16), (64, 4), (64, 4), (64, 4), (64, 4), (256, 16), (256, 16)]}


@pytest.mark.parametrize("kind,scale,tile,md", [("ddim", 7.5, 4, 2), ("2m", 7.5, 4, 2), ("unipc", 7.5, 4, 2), ("sde", 7.5, 4, 2)])
def test_seven_step_loops_vs_the_fp32_loop(tiny, plan, dev, gold, kind, scale, tile, md):
    """Every loop runs the strongest setting the tiny net allows -- tile 4 with max_downsample 2: all seven context blocks tiled,
    the 16 x 16 ones into 16 tiles -- because the final latent must sit further from the untiled loop than the loop bound for the
    test to tell an ignored key from an honoured one.  (Measured at the milder tile 8, max_downsample 1: the forward moves by
    6e-2, the seven-step latent by 1.06e-2 (DDIM) and 9.2e-3 (UniPC), too close to the bound of 1e-2 to resolve the feature; the
    forward tests cover that setting.)"""
    from lib.model_zoo.vd import hypertile_blocks, HyperTile
    net, sd = tiny
    xT, cs = _gold_case(gold, scale)
    sampler = _make(kind, net)
    call = {"eta": 0.0} if kind == "sde" else {}
    z, inter = _sample(sampler, dev, xT, cs, call=call, hypertile=tile, hypertile_max_downsample=md)
    assert len(sampler.ddim_timesteps) == 7
    assert inter["hypertile_tiles"] == TILES_TINY[(tile, md)]
    assert inter["hypertile_tiles"] == [(H * W, a * b) for _, H, W, a, b in hypertile_blocks(net.diffuser["image"], 16, 16, HyperTile(tile, md))]
    ref = hc.oracle_loop(sd, plan, sampler, kind, xT, cs, scale, tile, md)
    z_off, i_off = _sample(sampler, dev, xT, cs, call=call)
    err, moved = rel_l2(z, ref), rel_l2(z, z_off)
    print("%s s %.1f tile %d max_downsample %d: final latent vs the fp32 tiled loop %.3e; tiled vs untiled latent %.3e"
          % (kind, scale, tile, md, err, moved))
    assert "hypertile_tiles" not in i_off
    assert err < LATENT_TOL and moved > LATENT_TOL


@pytest.mark.parametrize("kind", ["ddim", "2m", "unipc", "sde"])
def test_graph_replay_eager_steps_and_a_fresh_sampler_agree_bitwise(tiny, dev, gold, monkeypatch, kind):
    net, _ = tiny
    xT, cs = _gold_case(gold)
    keys = {"seeds": [5, 6]} if kind == "sde" else {}
    shared = _make(kind, net)
    z_off0, i_off = _sample(shared, dev, xT, cs, **keys)                      # before any call with the key
    z_on, i_on = _sample(shared, dev, xT, cs, hypertile=8, **keys)
    z_off, _ = _sample(shared, dev, xT, cs, **keys)                           # an off-call behind an on-call: its own earlier bits
    assert torch.equal(z_off, z_off0) and not torch.equal(z_on, z_off) and "hypertile_tiles" not in i_off
    assert i_on["hypertile_tiles"] == TILES_TINY[(8, 1)]
    assert len(shared._static) == 2 and all(st["graph"] is not None for st in shared._static.values())
    assert torch.equal(_sample(shared, dev, xT, cs, hypertile=8, **keys)[0], z_on)             # the same call twice, on the kept graph
    for off_keys in (dict(hypertile=0), dict(hypertile=None, hypertile_max_downsample=2), dict(hypertile=16, hypertile_max_downsample=4)):
        assert torch.equal(_sample(shared, dev, xT, cs, **dict(keys, **off_keys))[0], z_off)
    z_two, i_two = _sample(shared, dev, xT, cs, hypertile=4, hypertile_max_downsample=2, **keys)       # another setting: another graph
    assert not torch.equal(z_two, z_on) and not torch.equal(z_two, z_off) and i_two["hypertile_tiles"] == TILES_TINY[(4, 2)]
    assert torch.equal(_sample(_make(kind, net), dev, xT, cs, hypertile=8, **keys)[0], z_on)          # a fresh sampler
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = _make(kind, net)
    assert not eager.use_graph
    assert torch.equal(_sample(eager, dev, xT, cs, hypertile=8, **keys)[0], z_on)
    assert torch.equal(_sample(eager, dev, xT, cs, hypertile=4, hypertile_max_downsample=2, **keys)[0], z_two)
    assert torch.equal(_sample(eager, dev, xT, cs, **keys)[0], z_off)


def test_multicontext_eager_ddim_and_single_steps_honour_the_key(tiny, dev, gold):
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    xT, cs = _gold_case(gold)
    g = torch.Generator().manual_seed(9)
    img = _ci((torch.randn((2, 50, 128), generator=g) * 0.5), (torch.randn((2, 50, 128), generator=g) * 0.5), 7.5, "image", ratio=0.6)
    s = _make("2m", net)
    multi = lambda **kw: s.sample_multicontext(steps=5, shape=SHAPE, x_info=dict({"type": "image", "xt": xT.half().to(dev)}, **kw),
                                               c_info_list=[dict(_on_dev(cs[0], dev), ratio=0.4), _on_dev(img, dev)], verbose=False)
    z_on, inter = multi(hypertile=8)
    z_off, _ = multi()
    assert inter["hypertile_tiles"] == TILES_TINY[(8, 1)] and rel_l2(z_on, z_off) > 1e-3 and torch.equal(multi(hypertile=8)[0], z_on)
    outs = []
    for keys in ({"hypertile": 8}, {"hypertile": 8, "hypertile_max_downsample": 1}, {}, {"hypertile": 0}):
        torch.manual_seed(3)
        outs.append(_sample(DDIMSampler(net), dev, xT, cs, steps=5, call={"eta": 0.5}, **keys)[0])     # the eager loop (eta > 0)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3]) and rel_l2(outs[0], outs[2]) > 1e-3
    s = DDIMSampler(net)
    s.make_schedule(5, verbose=False)
    t = torch.full((2,), int(s.ddim_timesteps[4]), dtype=torch.long, device=dev)
    x = xT.half().to(dev)
    c = _on_dev(cs[0], dev)
    step = lambda **kw: s.p_sample_ddim(dict({"type": "image", "x": x}, **kw), c, t, 4)[0]
    assert torch.equal(step(hypertile=0), step()) and rel_l2(step(hypertile=8), step()) > 1e-3


# ---- 6. interplay ----------------------------------------------------------------------------------------------------------------

def test_with_windows_deepcache_freeu_rescale_inpainting_pag_and_sag(tiny, dev, gold):
    """One loop each; every one runs on its kept graph, differs from its untiled twin and repeats its bits."""
    net, _ = tiny
    xT, cs = _gold_case(gold)
    g = torch.Generator().manual_seed(4)
    wide = torch.randn((2, 4, 16, 24), generator=g)
    mask = torch.zeros((2, 1, 16, 16))
    mask[:, :, :, :8] = 1
    cases = [
        (dict(window=16), wide, {}, 5),                      # the tiles are cut on the window's 16 x 16 grid, not the canvas' 16 x 24
        (dict(cache_interval=2, cache_depth=1), xT, {}, 5),
        (dict(freeu=(1.1, 1.2, 0.9, 0.8), inpaint_mask=mask.half().to(dev), x0=xT.half().to(dev)), xT, {"guidance_rescale": 0.7}, 5),
        (dict(pag_scale=3.0), xT, {}, 5),                    # the perturbed layer is the middle block: untiled
        (dict(pag_scale=3.0, pag_layers=(0, 2)), xT, {}, 5),  # a perturbed layer that is tiled too
        (dict(sag_scale=0.75), xT, {}, 4),                   # the map block (8 x 8) stays untiled at tile 8
    ]
    for keys, x0, c_keys, steps in cases:
        s = _make("2m", net)
        z_on, inter = _sample(s, dev, x0, cs, steps=steps, c_keys=c_keys, hypertile=8, **keys)
        z_off, _ = _sample(s, dev, x0, cs, steps=steps, c_keys=c_keys, **keys)
        assert inter["hypertile_tiles"] == TILES_TINY[(8, 1)], keys
        assert rel_l2(z_on, z_off) > 1e-3, keys
        assert torch.equal(_sample(s, dev, x0, cs, steps=steps, c_keys=c_keys, hypertile=8, **keys)[0], z_on), keys


def test_value_errors_on_the_device_path(tiny, dev, gold):
    from lib.model_zoo.vd import HyperTile, TokenMerge
    net, _ = tiny
    xT, cs = _gold_case(gold)
    s = _make("ddim", net)
    with pytest.raises(ValueError, match="hypertile.*divide"):
        _sample(s, dev, torch.zeros(2, 4, 16, 20), cs, hypertile=8)
    with pytest.raises(ValueError, match="hypertile.*tome"):
        _sample(s, dev, xT, cs, hypertile=8, tome_ratio=0.5)
    with pytest.raises(ValueError, match="hypertile.*sag"):
        _sample(s, dev, xT, cs, steps=4, hypertile=4, hypertile_max_downsample=2, sag_scale=0.75)
    with pytest.raises(ValueError, match="hypertile"):
        _sample(s, dev, xT, cs, hypertile=True)
    assert len(s._static) == 0
    x, ctx = _inputs(5, 2, False, True)
    with pytest.raises(ValueError, match="hypertile.*tome"):
        _fwd(net, dev, x, 500, ctx, 2, hypertile=HyperTile(8), tome=TokenMerge(0.5))
    with pytest.raises(ValueError, match="hypertile"):
        _fwd(net, dev, x, 500, ctx, 2, hypertile=8.0)
    with pytest.raises(ValueError, match="hypertile.*sag"):
        _fwd(net, dev, x, 500, ctx, 2, hypertile=HyperTile(4, 2), sag=torch.zeros((1, 2, 64), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="hypertile.*divide"):
        _fwd(net, dev, torch.zeros(2, 4, 16, 20), 500, ctx, 2, hypertile=8)
