"""SDE-DPM-Solver++(2M) on the GPU: the fused CFG + multistep + in-kernel noise update (vd_cfg_dpmpp_sde_step_dev_f16,
through the C ABI) against an fp64 formula with the noise of the numpy restatement (tests/test_philox_cpu.py), and
DPMSolverSDESampler against DPMSolverSampler (eta = 0, bitwise), against an fp64 loop on the CPU oracle (eta = 1), graph
replay and kept graphs, seeds, the RNG contract, inpainting and the sharding helper."""
import numpy as np
import pytest
import torch

from test_philox_cpu import normals_ref_batch
from vdtest_util import load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

LATENT_TOL = 1e-2            # the bound of test_dpm_solver_gpu.test_order2_tiny_vs_oracle
NOISE_ATOL = 2e-5            # of the generated normals (tests/test_philox_gpu.py)
SHAPE = [2, 4, 16, 16]
KSEEDS = [11, 2 ** 35 + 5, 2 ** 63 - 1]


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


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------

def _table(scale, eta=1.0):
    from lib.model_zoo.diffusion_utils import make_ddim_timesteps
    from lib.model_zoo.dpm_solver import dpmpp_sde_coef_table
    from oracle import vd_oracle as O
    return dpmpp_sde_coef_table(O.register_schedule()["alphas_cumprod"].numpy(),
                                make_ddim_timesteps("uniform", 10, 1000, verbose=False), eta=eta, scale=scale)


def _inputs(B, per, guided, seed):
    gen = torch.Generator().manual_seed(seed)
    n = B * per
    return torch.randn(n, generator=gen).half(), torch.randn(2 * n if guided else n, generator=gen).half()


def _run_kernel(dev, x_h, eps_h, B, per, guided, offset, alias, rows, seeds=KSEEDS, sde=True):
    """Two consecutive steps (rows[0] without history, rows[1] on it; draws 0 and 1) on views `offset` elements into larger
    allocations (misaligned for offset = 1: the scalar path).  Returns per step (x_next, p0, hist) on the host and the
    history the step started from."""
    from vd_hip import ops
    n = B * per

    def buf(m, dtype, fill=None):
        base = torch.empty((m + offset,), device=dev, dtype=dtype)
        if fill is not None:
            base.fill_(fill)
        return base[offset:]

    x = buf(n, torch.float16).view(B, per)
    x.copy_(x_h.view(B, per))
    eps = buf(eps_h.numel(), torch.float16)
    eps.copy_(eps_h)
    hist = buf(n, torch.float32, float("nan"))          # the first step must not read it
    p0 = buf(n, torch.float16)
    sd = torch.tensor(seeds, dtype=torch.int64, device=dev)
    out = []
    for draw, row in enumerate(rows):
        prev = hist.cpu().clone()
        coef = torch.from_numpy(np.ascontiguousarray(row)).to(dev)
        x_next = x if alias else buf(n, torch.float16).view(B, per)
        if sde:
            rng = torch.tensor([draw, 2], dtype=torch.int32, device=dev)
            ops.cfg_dpmpp_sde_step_dev(x, eps, coef, hist, sd, rng, guided=guided, x_next=x_next, pred_x0=p0)
        else:
            ops.cfg_dpmpp_step_dev(x, eps, coef, hist, guided=guided, x_next=x_next, pred_x0=p0)
        torch.cuda.synchronize()
        out.append((x_next.cpu().clone().reshape(-1), p0.cpu().clone(), hist.cpu().clone(), prev))
        x = x_next
    return out


@pytest.mark.parametrize("per", [105, 4096])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("alias", [False, True])
def test_kernel_vs_fp64_formula(dev, per, offset, guided, alias):
    B = 3
    tab = _table(7.5 if guided else 1.0)
    rows = (tab[-1], tab[5])
    assert rows[0][6] == 0 and rows[1][6] != 0 and rows[0][7] > 0 and rows[1][7] > 0
    x_h, eps_h = _inputs(B, per, guided, per + 7 * offset + 3 * guided + alias)
    steps = _run_kernel(dev, x_h, eps_h, B, per, guided, offset, alias, rows)
    n = B * per
    xd, ed = x_h.double(), eps_h.double()
    for draw, (row, (x_next, p0, hist, prev)) in enumerate(zip(rows, steps)):
        r = [float(v) for v in row.astype(np.float64)]
        z = torch.from_numpy(normals_ref_batch(KSEEDS, per, draw, 2)).reshape(-1)
        e = ed[:n] + r[0] * (ed[n:] - ed[:n]) if guided else ed
        x0 = (xd - r[2] * e) * r[1]
        d = r[5] * x0 + (r[6] * prev.double() if r[6] != 0 else 0.0)
        xn = r[3] * xd + r[4] * d + r[7] * z
        assert bool(torch.isfinite(x_next).all()) and bool(torch.isfinite(hist).all())
        torch.testing.assert_close(x_next.double(), xn, rtol=2 ** -10, atol=2e-4 + r[7] * NOISE_ATOL)
        torch.testing.assert_close(p0.double(), x0, rtol=2 ** -10, atol=2e-4)
        assert rel_l2(hist, x0) < 1e-6
        # the noise is really there: without it the step is off by about coef[7]
        assert rel_l2(x_next.double(), xn - r[7] * z) > 0.05 * r[7]
        xd = x_next.double()


@pytest.mark.parametrize("guided", [True, False])
def test_vector_and_scalar_paths_give_the_same_bits(dev, guided):
    B, per = 3, 4096
    tab = _table(7.5 if guided else 1.0)
    x_h, eps_h = _inputs(B, per, guided, 91 + guided)
    vec = _run_kernel(dev, x_h, eps_h, B, per, guided, 0, True, (tab[-1], tab[5]))
    sca = _run_kernel(dev, x_h, eps_h, B, per, guided, 1, True, (tab[-1], tab[5]))
    for a, b in zip(vec, sca):
        for u, v in zip(a[:3], b[:3]):
            assert torch.equal(u, v)


@pytest.mark.parametrize("per,offset", [(105, 0), (4096, 0), (4096, 1)])
@pytest.mark.parametrize("guided", [True, False])
def test_zero_noise_coefficient_is_the_2m_kernel_bitwise(dev, per, offset, guided):
    B = 3
    tab = _table(7.5 if guided else 1.0, eta=0.0)
    assert (tab[:, 7] == 0).all()
    x_h, eps_h = _inputs(B, per, guided, 17 + per + offset)
    sde = _run_kernel(dev, x_h, eps_h, B, per, guided, offset, False, (tab[-1], tab[5]))
    ref = _run_kernel(dev, x_h, eps_h, B, per, guided, offset, False, (tab[-1], tab[5]), sde=False)
    for a, b in zip(sde, ref):
        for u, v in zip(a[:3], b[:3]):
            assert torch.equal(u, v)


@pytest.mark.parametrize("per", [105, 4096])
def test_rows_of_a_batch_equal_the_samples_run_alone(dev, per):
    B, guided = 3, True
    tab = _table(7.5)
    rows = (tab[-1], tab[5])
    x_h, eps_h = _inputs(B, per, guided, 23 + per)
    whole = _run_kernel(dev, x_h, eps_h, B, per, guided, 0, True, rows)
    eu, ec = eps_h[:B * per].view(B, per), eps_h[B * per:].view(B, per)
    for b in range(B):
        one = _run_kernel(dev, x_h.view(B, per)[b].clone(), torch.cat([eu[b], ec[b]]), 1, per, guided, 0, True, rows,
                          seeds=KSEEDS[b:b + 1])
        for w, o in zip(whole, one):
            for u, v in zip(w[:3], o[:3]):
                assert torch.equal(u.view(B, per)[b], v.view(-1))


def test_kernel_argument_checks(dev):
    from vd_hip import ops
    from vd_hip.loader import VdHipError
    f16 = dict(device=dev, dtype=torch.float16)
    x, eps = torch.zeros((2, 16), **f16), torch.zeros((4, 16), **f16)
    coef = torch.zeros(8, device=dev)
    hist = torch.zeros((2, 16), device=dev)
    seeds = torch.zeros(2, dtype=torch.int64, device=dev)
    rng = torch.zeros(2, dtype=torch.int32, device=dev)
    ops.cfg_dpmpp_sde_step_dev(x, eps, coef, hist, seeds, rng, guided=True, x_next=x)
    with pytest.raises(VdHipError):
        ops.cfg_dpmpp_sde_step_dev(x, eps, coef, hist, seeds[:1], rng, guided=True, x_next=x)
    with pytest.raises(VdHipError):
        ops.cfg_dpmpp_sde_step_dev(x, eps, coef, hist, seeds.int(), rng, guided=True, x_next=x)
    with pytest.raises(VdHipError):
        ops.cfg_dpmpp_sde_step_dev(x, eps, coef, hist, seeds, rng.long(), guided=True, x_next=x)
    with pytest.raises(VdHipError):
        ops.cfg_dpmpp_sde_step_dev(x, eps, coef[:7], hist, seeds, rng, guided=True, x_next=x)
    with pytest.raises(VdHipError):
        ops.cfg_dpmpp_sde_step_dev(x, eps[:2], coef, hist, seeds, rng, guided=True, x_next=x)


# ---- 2. the sampler -----------------------------------------------------------------------------------------------------

def _case(dev, seed, shape=SHAPE):
    g = torch.Generator().manual_seed(seed)
    xT = torch.randn(shape, generator=g).half().to(dev)
    c = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half().to(dev)
    u = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half().to(dev)
    return xT, c, u


def _t2i(sampler, xT, c, u, scale, steps, seeds=None, **kw):
    x_info = {"type": "image"}
    if xT is not None:
        x_info["xt"] = xT
    if seeds is not None:
        x_info["seeds"] = seeds
    z, _ = sampler.sample(steps=steps, shape=list(c.shape[:1]) + SHAPE[1:], x_info=x_info, c_info=_ci(c, u, scale),
                          verbose=False, **kw)
    return z


def test_eta0_is_the_2m_sampler_bitwise(tiny, dev):
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    net, _ = tiny
    xT, c, u = _case(dev, 5)
    z_2m = _t2i(DPMSolverSampler(net), xT, c, u, 7.5, 8)
    assert torch.equal(_t2i(DPMSolverSDESampler(net, eta=0.0), xT, c, u, 7.5, 8), z_2m)
    assert torch.equal(_t2i(DPMSolverSDESampler(net), xT, c, u, 7.5, 8, seeds=[1, 2], eta=0.0), z_2m)


def test_eta1_tiny_vs_fp64_loop_on_the_oracle(tiny, dev, gold):
    """The sampler's loop in float64 around the fp32 CPU oracle UNet, driven by the table the sampler used and the
    restatement's noise (draw = step number, stream 2)."""
    from lib.model_zoo.dpm_solver import DPMSolverSDESampler, dpmpp_sde_coef_table
    from oracle import vd_oracle as O
    net, sd = tiny
    plan = O.unet_plan(**meta()["unet2d"])
    xT = torch.from_numpy(gold["xT"]).float()
    c, u = torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"])
    seeds, scale, steps = [41, 2 ** 33 + 9], 7.5, 10
    sampler = DPMSolverSDESampler(net)
    z = _t2i(sampler, xT.half().to(dev), c.half().to(dev), u.half().to(dev), scale, steps, seeds=seeds)
    ts = sampler.ddim_timesteps
    tab = dpmpp_sde_coef_table(sampler.alphas_cumprod, ts, eta=1.0, order=sampler.order,
                               lower_order_final=sampler.lower_order_final, scale=scale).astype(np.float64)
    assert (tab[:, 7] > 0).all()
    per = int(np.prod(SHAPE[1:]))
    x, hist = xT.double(), None
    cs = [("text", torch.cat([u, c]).float(), 1.0)]
    for draw, i in enumerate(reversed(range(len(ts)))):
        r = tab[i]
        t = torch.full((2 * x.shape[0],), int(ts[i]), dtype=torch.long)
        with torch.no_grad():
            e_u, e_c = O.apply_model_multicontext(sd, plan, torch.cat([x, x]).float(), t, cs, "image", "image").double().chunk(2)
        e = e_u + r[0] * (e_c - e_u)
        x0 = (x - r[2] * e) * r[1]
        d = r[5] * x0 + (r[6] * hist if r[6] != 0 else 0.0)
        zn = torch.from_numpy(normals_ref_batch(seeds, per, draw, 2)).reshape(x.shape)
        x, hist = r[3] * x + r[4] * d + r[7] * zn, x0
    err = rel_l2(z, x)
    print("10-step SDE-DPM-Solver++(2M) rel-L2 vs the fp64 loop on the oracle: %.3e" % err)
    assert err < LATENT_TOL


def test_graph_replay_matches_eager_bitwise(tiny, dev, monkeypatch):
    from lib.model_zoo.dpm_solver import DPMSolverSDESampler
    net, _ = tiny
    xT, c, u = _case(dev, 5)
    z_graph = _t2i(DPMSolverSDESampler(net), xT, c, u, 7.5, 8, seeds=[3, 4])
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = DPMSolverSDESampler(net)
    assert not eager.use_graph
    assert torch.equal(z_graph, _t2i(eager, xT, c, u, 7.5, 8, seeds=[3, 4]))


def test_kept_graph_reused_with_other_seeds_steps_and_context(tiny, dev):
    from lib.model_zoo.dpm_solver import DPMSolverSDESampler
    net, _ = tiny
    shared = DPMSolverSDESampler(net)
    a, b = _case(dev, 6), _case(dev, 7)
    z_a = _t2i(shared, *a, 7.5, 6, seeds=[1, 2])
    st = next(iter(shared._static.values()))
    graph = st["graph"]
    assert graph is not None and st["seeds"].dtype == torch.int64 and st["rng"].dtype == torch.int32
    assert st["coef"].numel() == 8 and st["rng"].tolist() == [len(shared.ddim_timesteps) - 1, 2]   # {last draw, stream}
    z_b = _t2i(shared, *b, 3.0, 11, seeds=[2 ** 40, 9])
    assert len(shared._static) == 1 and st["graph"] is graph       # replayed, not captured again
    assert st["seeds"].tolist() == [2 ** 40, 9] and st["rng"].tolist() == [len(shared.ddim_timesteps) - 1, 2]
    assert torch.equal(z_b, _t2i(DPMSolverSDESampler(net), *b, 3.0, 11, seeds=[2 ** 40, 9]))
    assert torch.equal(z_a, _t2i(DPMSolverSDESampler(net), *a, 7.5, 6, seeds=[1, 2]))
    assert rel_l2(z_a, z_b) > 0.1


def test_seeds_decide_the_result_and_the_device_generator_is_untouched(tiny, dev):
    from lib.model_zoo.dpm_solver import DPMSolverSDESampler
    net, _ = tiny
    _, c, u = _case(dev, 8)
    sampler = DPMSolverSDESampler(net)
    torch.manual_seed(123)
    before = torch.cuda.get_rng_state(dev)
    z1 = _t2i(sampler, None, c, u, 7.5, 6, seeds=[10, 11])             # x_T from the seeds too
    assert torch.equal(torch.cuda.get_rng_state(dev), before)
    torch.manual_seed(456)                                              # torch's generator plays no part
    z2 = _t2i(sampler, None, c, u, 7.5, 6, seeds=torch.tensor([10, 11]))
    assert torch.equal(z1, z2)
    z3 = _t2i(sampler, None, c, u, 7.5, 6, seeds=[10, 12])
    assert rel_l2(z3[1], z1[1]) > 0.1
    assert rel_l2(z3[0], z1[0]) < 5e-3         # sample 0 kept its seed: same noise, same image within fp16 tolerance
    # the forward-process noise of the x0 path comes from the seeds as well (stream 1)
    x0 = (torch.randn(SHAPE, generator=torch.Generator().manual_seed(2)) * 0.5).half().to(dev)
    before = torch.cuda.get_rng_state(dev)
    runs = [sampler.sample(steps=6, shape=SHAPE, x_info={"type": "image", "x0": x0, "x0_forward_timesteps": 4,
                                                         "seeds": [10, 11]}, c_info=_ci(c, u, 7.5), verbose=False)[0]
            for _ in range(2)]
    assert torch.equal(torch.cuda.get_rng_state(dev), before) and torch.equal(runs[0], runs[1])
    # temperature is the noise scale
    z_cold = _t2i(sampler, z1.new_zeros(SHAPE) + 1, c, u, 7.5, 6, seeds=[10, 11], temperature=0.0)
    z_2m = _t2i(sampler, z1.new_zeros(SHAPE) + 1, c, u, 7.5, 6, seeds=[10, 11], eta=0.0)
    assert rel_l2(z_cold, z_2m) > 1e-3         # eta = 1 without noise is not the ODE solver: other x and D coefficients


def test_interleaved_with_ddim_and_2m_on_one_model(tiny, dev):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler, DPMSolverSDESampler
    net, _ = tiny
    ddim, dpm, sde = DDIMSampler(net), DPMSolverSampler(net), DPMSolverSDESampler(net)
    cases = [_case(dev, 20 + k) for k in range(2)]
    outs = []
    for k, args in enumerate(cases):
        outs.append((_t2i(ddim, *args, 7.5, 5 + k), _t2i(sde, *args, 7.5, 6 + k, seeds=[k, k + 5]),
                     _t2i(dpm, *args, 7.5, 7 + k)))
    for k, args in enumerate(cases):
        assert rel_l2(outs[k][0], _t2i(DDIMSampler(net), *args, 7.5, 5 + k)) < 5e-3, k
        assert torch.equal(outs[k][1], _t2i(DPMSolverSDESampler(net), *args, 7.5, 6 + k, seeds=[k, k + 5])), k
        assert rel_l2(outs[k][2], _t2i(DPMSolverSampler(net), *args, 7.5, 7 + k)) < 5e-3, k


def test_inpainting_returns_the_known_region_bitwise(tiny, dev):
    from lib.model_zoo.dpm_solver import DPMSolverSDESampler
    net, _ = tiny
    _, c, u = _case(dev, 9)
    g = torch.Generator().manual_seed(4)
    x0 = (torch.randn(SHAPE, generator=g) * 0.5).half().to(dev)
    mask = torch.ones((2, 1, 16, 16))
    mask[..., :6, :] = 0                         # keep the top rows
    mask = mask.half().to(dev)
    z, _ = DPMSolverSDESampler(net).sample(steps=6, shape=SHAPE, x_info={"type": "image", "x0": x0, "inpaint_mask": mask,
                                                                        "seeds": [5, 6]},
                                           c_info=_ci(c, u, 7.5), verbose=False)
    keep = (mask == 0).expand_as(x0)
    assert torch.equal(z[keep], x0[keep])
    assert rel_l2(z[~keep], x0[~keep]) > 0.1 and bool(torch.isfinite(z).all())


def test_sharded_world1_matches_direct_sample(tiny, dev, gold):
    from lib.model_zoo import sharded
    from lib.model_zoo.dpm_solver import DPMSolverSDESampler
    net, _ = tiny
    ct = _ci(T(gold["c_text"], dev), T(gold["u_text"], dev), 7.5)
    seed, steps = 3, 6
    imgs = sharded.vd_sample_sharded(net, DPMSolverSDESampler(net), steps, SHAPE, [dict(ct)], seed, guidance_scale=7.5,
                                     eta=1.0)
    xT = sharded.draw_initial_latent(SHAPE, seed).to(dev)
    z, _ = DPMSolverSDESampler(net).sample(steps=steps, shape=SHAPE, x_info={"type": "image", "xt": xT,
                                                                            "seeds": sharded.sample_seeds(seed, 0, 2)},
                                           c_info=dict(ct), eta=1.0, verbose=False)
    ref = net.vae_decode(z, which="image")
    assert imgs.shape == ref.shape and rel_l2(imgs, ref) < 2e-3
    # and the seeds matter: another batch seed, same x_T
    z2, _ = DPMSolverSDESampler(net).sample(steps=steps, shape=SHAPE, x_info={"type": "image", "xt": xT,
                                                                             "seeds": sharded.sample_seeds(seed + 1, 0, 2)},
                                            c_info=dict(ct), eta=1.0, verbose=False)
    assert rel_l2(z2, z) > 0.05
