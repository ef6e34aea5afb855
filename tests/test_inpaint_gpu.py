"""Inpainting (blended latent diffusion) on the GPU: the masked-blend kernel (vd_masked_blend_f16, through the C ABI)
against an fp64 formula, masked DDIM and DPM-Solver++ loops against the fp32 CPU oracle driven by the tables the sampler
used, hard-mask exactness, kept graphs, the RNG contract and the sharding helper."""
import numpy as np
import pytest
import torch

from vdtest_util import full_vd_cfg, load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

LATENT_TOL = 1e-2
SHAPE = [2, 4, 16, 16]


def T(a, dev, dtype=torch.float16):
    return torch.from_numpy(np.asarray(a)).to(dev).to(dtype)


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
def gold():
    return load_gold("ddim_tiny.npz")


def _ci(c, u, scale, ctype="text", **kw):
    return dict({"type": ctype, "conditioning": c, "unconditional_conditioning": u, "unconditional_guidance_scale": scale},
                **kw)


def _on_dev(c, dev):
    return dict(c, conditioning=c["conditioning"].half().to(dev),
                unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))


def _soft_mask(batch, seed, hw=(16, 16)):
    """fp16-representable soft mask with exact 0 and 1 regions."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand((batch, 1) + tuple(hw), generator=g)
    m[..., : hw[0] // 4, :] = 0
    m[..., -hw[0] // 4:, :] = 1
    return m.half().float()


def _oracle(sd, plan, sampler, x, contexts, scale, x0, noise, mask, k=None):
    """The sampler's loop (DDIM with eta = 0, or DPM-Solver++ from dpmpp_coef_table) in fp32 on the CPU oracle, with the
    blend m x + (1 - m) (ca x0 + cn noise) after every step; the schedule is the sampler's last call's (its first k
    entries on the x0 + x0_forward_timesteps path)."""
    from lib.model_zoo.ddim import inpaint_blend_table
    from lib.model_zoo.diffusion_utils import make_ddim_sampling_parameters
    from lib.model_zoo.dpm_solver import DPMSolverSampler, dpmpp_coef_table
    from oracle import vd_oracle as O
    ts = sampler.ddim_timesteps if k is None else sampler.ddim_timesteps[:k]
    blend = inpaint_blend_table(sampler.alphas_cumprod, ts).astype(np.float64)
    dpm = isinstance(sampler, DPMSolverSampler)
    if dpm:
        tab = dpmpp_coef_table(sampler.alphas_cumprod, ts, order=sampler.order,
                               lower_order_final=sampler.lower_order_final, scale=scale).astype(np.float64)
    else:
        _, a_t, a_prev = make_ddim_sampling_parameters(sampler.alphas_cumprod, ts, 0.0, verbose=False)
    x, hist = x.float(), None
    x0, noise, mask = x0.float(), noise.float(), mask.float()
    cs = [(c["type"], torch.cat([c["unconditional_conditioning"], c["conditioning"]]).float(), c.get("ratio", 1.0))
          for c in contexts]
    for i in reversed(range(len(ts))):
        t = torch.full((2 * x.shape[0],), int(ts[i]), dtype=torch.long)
        with torch.no_grad():
            e_u, e_c = O.apply_model_multicontext(sd, plan, torch.cat([x, x]), t, cs, "image", "image").chunk(2)
        e = e_u + scale * (e_c - e_u)
        if dpm:
            r = tab[i]
            p0 = (x - r[2] * e) * r[1]
            d = r[5] * p0 + (r[6] * hist if r[6] != 0 else 0.0)
            x, hist = r[3] * x + r[4] * d, p0
        else:
            p0 = (x - np.sqrt(1 - a_t[i]) * e) / np.sqrt(a_t[i])
            x = np.sqrt(a_prev[i]) * p0 + np.sqrt(1 - a_prev[i]) * e
        x = mask * x + (1 - mask) * (blend[i, 0] * x0 + blend[i, 1] * noise)
    return x


def _samplers():
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    return {"ddim": DDIMSampler, "dpm": DPMSolverSampler}


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------

def _ulp16(r):
    a = r.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


@pytest.mark.parametrize("B,Bm,hw,offset", [(2, 1, 4096, 0), (2, 2, 4096, 0), (3, 3, 63, 0), (3, 1, 63, 0),
                                            (2, 2, 4096, 1), (2, 1, 64, 1)])
@pytest.mark.parametrize("alias", [False, True])
def test_kernel_vs_fp64_formula(dev, B, Bm, hw, offset, alias):
    from lib.model_zoo.ddim import inpaint_blend_table
    from lib.model_zoo.diffusion_utils import make_ddim_timesteps
    from oracle import vd_oracle as O
    from vd_hip import ops
    C = 4
    n = B * C * hw
    gen = torch.Generator().manual_seed(B * 1000 + Bm * 100 + hw + offset + 7 * alias)
    tab = inpaint_blend_table(O.register_schedule()["alphas_cumprod"].numpy(),
                              make_ddim_timesteps("uniform", 10, 1000, verbose=False))

    def buf(vals):      # a view `offset` elements into a larger allocation: misaligned for offset = 1
        base = torch.empty((vals.numel() + offset,), device=dev, dtype=torch.float16)
        v = base[offset:].view(vals.shape)
        v.copy_(vals.half())
        return v

    x0 = buf(torch.randn((B, C, hw), generator=gen))
    nz = buf(torch.randn((B, C, hw), generator=gen))
    soft = torch.rand((Bm, 1, hw), generator=gen)
    for row, mvals in ((tab[4], soft), (tab[0], soft), (tab[7], torch.ones_like(soft)), (tab[0], torch.zeros_like(soft))):
        x = buf(torch.randn((B, C, hw), generator=gen))
        mask = buf(mvals)
        xd, m = x.double().clone(), mask.double()
        coef = torch.from_numpy(row).to(dev)
        out = x if alias else buf(torch.zeros((B, C, hw)))
        ops.masked_blend(x, x0, nz, mask, coef, out=out)
        torch.cuda.synchronize()
        r = [float(v) for v in row]
        ref = m * xd + (1 - m) * (r[0] * x0.double() + r[1] * nz.double())
        assert out.shape == (B, C, hw) and bool(torch.isfinite(out).all())
        assert bool(((out.double() - ref).abs() <= _ulp16(ref)).all()), float((out.double() - ref).abs().max())
        if bool((mvals == 1).all()):
            assert torch.equal(out, xd.half())                    # m = 1: x bit for bit
        if bool((mvals == 0).all()) and r == [1.0, 0.0]:
            assert torch.equal(out, x0)                           # m = 0 on the last row: x0 bit for bit


# ---- 2. loops against the oracle ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ddim", "dpm"])
def test_masked_loops_tiny_vs_oracle(tiny, dev, gold, name):
    from oracle import vd_oracle as O
    net, sd = tiny
    plan = O.unet_plan(**meta()["unet2d"])
    sampler = _samplers()[name](net)
    xT, x0, qn = (torch.from_numpy(gold[k]).half().float() for k in ("xT", "x0", "q_noise"))
    ct = _ci(torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"]), 7.5)
    ci = _ci(torch.from_numpy(gold["c_img"]), torch.from_numpy(gold["u_img"]), 7.5, "image")
    m2, m1 = _soft_mask(2, 1), _soft_mask(1, 2)

    # 10 steps from x_T, per-sample mask; the blend noise is x_T itself
    x_info = {"type": "image", "xt": xT.half().to(dev), "x0": x0.half().to(dev), "inpaint_mask": m2.to(dev)}
    z, inter = sampler.sample(steps=10, shape=SHAPE, x_info=x_info, c_info=_on_dev(ct, dev), verbose=False)
    zref = _oracle(sd, plan, sampler, xT, [ct], 7.5, x0, xT, m2)
    assert rel_l2(z, zref) < LATENT_TOL, name
    assert torch.equal(inter["pred_xt"][-1], z)        # the logged latents are the blended ones

    # dual context (ratios 0.4 / 0.6), broadcast mask
    mc = [dict(ct, ratio=0.4), dict(ci, ratio=0.6)]
    x_info = {"type": "image", "xt": xT.half().to(dev), "x0": x0.half().to(dev), "inpaint_mask": m1.to(dev)}
    z, _ = sampler.sample_multicontext(steps=10, shape=SHAPE, x_info=x_info, c_info_list=[_on_dev(c, dev) for c in mc],
                                       verbose=False)
    assert rel_l2(z, _oracle(sd, plan, sampler, xT, mc, 7.5, x0, xT, m1)) < LATENT_TOL, name

    # the partial schedule: x0 + x0_forward_timesteps + x0_noise, the blend noise is x0_noise
    x_info = {"type": "image", "x0": x0.half().to(dev), "x0_forward_timesteps": 3, "x0_noise": qn.half().to(dev),
              "inpaint_mask": m1.to(dev)}
    z, _ = sampler.sample(steps=10, shape=SHAPE, x_info=x_info, c_info=_on_dev(ct, dev), verbose=False)
    ac = sampler.alphas_cumprod.astype(np.float64)
    t3 = int(sampler.ddim_timesteps[3])
    xs = float(np.sqrt(np.float32(ac[t3]))) * x0 + float(np.sqrt(1 - np.float32(ac[t3]))) * qn
    assert rel_l2(z, _oracle(sd, plan, sampler, xs, [ct], 7.5, x0, qn, m1, k=3)) < LATENT_TOL, name


def test_masked_dpm_full_width_vs_oracle(dev):
    """Full-width UNet, 32x32 latent, B = 2, 15 guided DPM-Solver++(2M) steps with a soft per-sample mask."""
    from lib.model_zoo import get_model
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    from oracle import vd_oracle as O
    net = get_model()(full_vd_cfg(with_vae=False), verbose=False)
    sd = synth_into(net, 7)
    net = net.half()
    net.to(dev)
    g = torch.Generator().manual_seed(43)
    xT = torch.randn((2, 4, 32, 32), generator=g).half().float()
    x0 = torch.randn((2, 4, 32, 32), generator=g).half().float()
    c = torch.randn((2, 77, 768), generator=g) * 0.5
    u = torch.randn((2, 77, 768), generator=g) * 0.5
    m = _soft_mask(2, 3, (32, 32))
    sampler = DPMSolverSampler(net)
    x_info = {"type": "image", "xt": xT.half().to(dev), "x0": x0.half().to(dev), "inpaint_mask": m.to(dev)}
    z, _ = sampler.sample(steps=15, shape=[2, 4, 32, 32], x_info=x_info, c_info=_ci(c.half().to(dev), u.half().to(dev), 7.5),
                          verbose=False)
    err = rel_l2(z, _oracle(sd, O.unet_plan(), sampler, xT, [_ci(c, u, 7.5)], 7.5, x0, xT, m))
    print("15-step masked DPM-Solver++(2M) rel-L2 vs fp32 oracle: %.3e" % err)
    assert err < LATENT_TOL


# ---- 3. hard masks ------------------------------------------------------------------------------------------------------

def _case(dev, seed, shape=tuple(SHAPE)):
    g = torch.Generator().manual_seed(seed)
    xT = torch.randn(shape, generator=g).half().to(dev)
    x0 = torch.randn(shape, generator=g).half().to(dev)
    c = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half().to(dev)
    u = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half().to(dev)
    return xT, x0, c, u


def _run(sampler, xT, x0, c, u, scale, steps, mask=None, seed=0, eta=0.):
    x_info = {"type": "image", "xt": xT}
    if mask is not None:
        x_info.update(x0=x0, inpaint_mask=mask)
    torch.manual_seed(seed)
    z, _ = sampler.sample(steps=steps, shape=list(xT.shape), x_info=x_info, c_info=_ci(c, u, scale), eta=eta,
                          verbose=False)
    return z


@pytest.mark.parametrize("name,eta", [("ddim", 0.), ("ddim", 0.5), ("dpm", 0.)])
def test_hard_mask_keeps_x0_and_all_ones_is_unmasked(tiny, dev, name, eta):
    net, _ = tiny
    cls = _samplers()[name]
    xT, x0, c, u = _case(dev, 11)
    hard = (torch.rand((2, 1, 16, 16), generator=torch.Generator().manual_seed(12)) > 0.5).to(dev)
    s = cls(net)
    z = _run(s, xT, x0, c, u, 7.5, 8, mask=hard, seed=5, eta=eta)
    keep = (~hard).expand_as(z)
    assert bool(keep.any()) and torch.equal(z[keep], x0[keep])       # the known region is x0 bit for bit
    assert rel_l2(z[~keep], x0[~keep]) > 0.1
    ones = torch.ones((1, 1, 16, 16), device=dev, dtype=torch.bool)
    z1 = _run(cls(net), xT, x0, c, u, 7.5, 8, mask=ones, seed=5, eta=eta)
    z_plain = _run(cls(net), xT, x0, c, u, 7.5, 8, seed=5, eta=eta)
    assert torch.equal(z1, z_plain)


# ---- 4. kept graphs -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ddim", "dpm"])
def test_kept_graph_masked_unmasked_masked(tiny, dev, name):
    """Masked A, unmasked B, masked C (other mask, x0, step count and scale) on one sampler == fresh samplers; C replays
    A's kept graph without capturing again, B captures its own."""
    net, _ = tiny
    cls = _samplers()[name]
    shared = cls(net)
    captures = []
    real_capture = shared._capture
    shared._capture = lambda body: captures.append(1) or real_capture(body)
    a, b, cc = _case(dev, 30), _case(dev, 31), _case(dev, 32)
    ma, mc = _soft_mask(2, 33).to(dev), _soft_mask(2, 34).to(dev)
    z_a = _run(shared, *a, 7.5, 6, mask=ma)
    st_a = next(st for st in shared._static.values() if "mask" in st)
    graph_a = st_a["graph"]
    assert graph_a is not None and len(captures) == 1
    z_b = _run(shared, *b, 7.5, 5)
    assert len(shared._static) == 2 and len(captures) == 2
    st_b = next(st for st in shared._static.values() if "mask" not in st)
    assert st_b["graph"] is not graph_a
    z_c = _run(shared, *cc, 3.0, 11, mask=mc)
    assert len(captures) == 2 and st_a["graph"] is graph_a and len(shared._static) == 2
    assert rel_l2(z_a, _run(cls(net), *a, 7.5, 6, mask=ma)) < 5e-3
    assert rel_l2(z_b, _run(cls(net), *b, 7.5, 5)) < 5e-3
    assert rel_l2(z_c, _run(cls(net), *cc, 3.0, 11, mask=mc)) < 5e-3
    assert rel_l2(z_a, z_c) > 0.1


# ---- 5. RNG / 6. sharding -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ddim", "dpm"])
@pytest.mark.parametrize("flow", ["random", "x0_forward"])
def test_rng_use_matches_unmasked_call(tiny, dev, gold, name, flow):
    net, _ = tiny
    cls = _samplers()[name]
    ct = _ci(T(gold["c_text"], dev), T(gold["u_text"], dev), 7.5)
    x0 = T(gold["x0"], dev)
    base = {"type": "image"} if flow == "random" else {"type": "image", "x0": x0, "x0_forward_timesteps": 3}
    after = []
    for masked in (False, True):
        x_info = dict(base)
        if masked:
            x_info.update(x0=x0, inpaint_mask=_soft_mask(1, 40).to(dev))
        torch.manual_seed(77)
        cls(net).sample(steps=6, shape=SHAPE, x_info=x_info, c_info=dict(ct), verbose=False)
        after.append(torch.randn(8, device=dev))
    assert torch.equal(after[0], after[1])


def test_sharded_world1_matches_direct_masked_sample(tiny, dev, gold):
    from lib.app_ops import latent_mask
    from lib.model_zoo import sharded
    from lib.model_zoo.ddim import DDIMSampler
    net, _ = tiny
    ct = _ci(T(gold["c_text"], dev), T(gold["u_text"], dev), 7.5)
    shape, seed, steps = SHAPE, 3, 6
    images = torch.rand((2, 3, 32, 32), generator=torch.Generator().manual_seed(50)).to(dev)
    pix = torch.zeros((1, 1, 32, 32), device=dev)
    pix[..., 5:19, 9:27] = 1
    imgs = sharded.vd_sample_sharded(net, DDIMSampler(net), steps, shape, [dict(ct)], seed, guidance_scale=7.5,
                                     images=images, mask=pix)
    x_T = sharded.draw_initial_latent(shape, seed).to(dev)
    post = sharded.draw_initial_latent(shape, seed + 1).to(dev)
    x0 = net.vae_encode(images, which="image", noise=post)
    x_info = {"type": "image", "xt": x_T, "x0": x0, "inpaint_mask": latent_mask(pix, mode="max", factor=2)}
    z, _ = DDIMSampler(net).sample(steps=steps, shape=shape, x_info=x_info, c_info=dict(ct), verbose=False)
    ref = net.vae_decode(z, which="image")
    assert imgs.shape == ref.shape and rel_l2(imgs, ref) < 2e-3
