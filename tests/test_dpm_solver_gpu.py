"""DPM-Solver++(2M) on the GPU: the fused CFG + multistep kernel (vd_cfg_dpmpp_step_dev_f16, through the C ABI) against
an fp64 torch formula, and DPMSolverSampler against DDIMSampler (order 1) and against the fp32 CPU oracle driven by the
same coefficient table (order 2); the bits of every fused sampler step against tests/golden/sampler_step_bits.json; graph
replay and kept graphs, the RNG contract and the sharding helper."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from vdtest_util import GOLD, full_vd_cfg, load_gold, meta, rel_l2, synth_into, tiny_vd_cfg

pytestmark = pytest.mark.gpu

LATENT_TOL = 1e-2


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


def _oracle_dpm(sd, plan, sampler, xT, contexts, scale, x_type="image"):
    """The solver loop in fp32 on the CPU oracle, driven by the table the sampler used for its last call."""
    from lib.model_zoo.dpm_solver import dpmpp_coef_table
    from oracle import vd_oracle as O
    ts = sampler.ddim_timesteps
    tab = torch.from_numpy(dpmpp_coef_table(sampler.alphas_cumprod, ts, order=sampler.order,
                                            lower_order_final=sampler.lower_order_final, scale=scale))
    x, hist = xT.float(), None
    for i in reversed(range(len(ts))):
        row = [float(v) for v in tab[i]]
        b = x.shape[0]
        t = torch.full((2 * b,), int(ts[i]), dtype=torch.long)
        cs = [(c["type"], torch.cat([c["unconditional_conditioning"], c["conditioning"]]).float(), c.get("ratio", 1.0))
              for c in contexts]
        with torch.no_grad():
            e_u, e_c = O.apply_model_multicontext(sd, plan, torch.cat([x, x]), t, cs, x_type, "image").chunk(2)
        e = e_u + row[0] * (e_c - e_u)
        x0 = (x - row[2] * e) * row[1]
        d = row[5] * x0 + (row[6] * hist if row[6] != 0 else 0.0)
        x, hist = row[3] * x + row[4] * d, x0
    return x


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------

def _kernel_case(dev, n, guided, offset, alias, gen):
    from lib.model_zoo.diffusion_utils import make_ddim_timesteps
    from lib.model_zoo.dpm_solver import dpmpp_coef_table
    from oracle import vd_oracle as O
    from vd_hip import ops
    scale = 7.5 if guided else 1.0
    tab = dpmpp_coef_table(O.register_schedule()["alphas_cumprod"].numpy(),
                           make_ddim_timesteps("uniform", 10, 1000, verbose=False), scale=scale)
    ne = 2 * n if guided else n

    def buf(m, dtype, fill=None):   # a view `offset` elements into a larger allocation: misaligned for offset = 1
        base = torch.empty((m + offset,), device=dev, dtype=dtype)
        if fill is not None:
            base.fill_(fill)
        return base[offset:]

    x = buf(n, torch.float16)
    x.copy_(torch.randn(n, generator=gen).half())
    eps = buf(ne, torch.float16)
    eps.copy_(torch.randn(ne, generator=gen).half())
    hist = buf(n, torch.float32, float("nan"))
    p0 = buf(n, torch.float16)
    xd, ed = x.double(), eps.double()
    for row in (tab[-1], tab[5]):        # the first step (no history: NaNs must not be read), then a second-order step
        r = [float(v) for v in row.astype(np.float64)]
        prev = hist.double().clone()
        coef = torch.from_numpy(row).to(dev)
        x_next = x if alias else buf(n, torch.float16)
        ops.cfg_dpmpp_step_dev(x, eps, coef, hist, guided=guided, x_next=x_next, pred_x0=p0)
        torch.cuda.synchronize()
        e = ed[:n] + r[0] * (ed[n:] - ed[:n]) if guided else ed
        x0 = (xd - r[2] * e) * r[1]
        d = r[5] * x0 + (r[6] * prev if r[6] != 0 else 0.0)
        xn = r[3] * xd + r[4] * d
        assert bool(torch.isfinite(x_next).all()) and bool(torch.isfinite(hist).all())
        torch.testing.assert_close(x_next.double(), xn, rtol=2 ** -10, atol=2e-4)
        torch.testing.assert_close(p0.double(), x0, rtol=2 ** -10, atol=2e-4)
        assert rel_l2(hist, x0) < 1e-6
        x, xd = x_next, x_next.double()
    return r


@pytest.mark.parametrize("n,offset", [(65536, 0), (4099, 0), (4099, 1)])
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("alias", [False, True])
def test_kernel_vs_fp64_formula(dev, n, offset, guided, alias):
    gen = torch.Generator().manual_seed(n + 7 * offset + 3 * guided + alias)
    r = _kernel_case(dev, n, guided, offset, alias, gen)
    assert r[6] != 0          # the second call really was a second-order step


@pytest.mark.parametrize("family", ["solver", "ddim"])
def test_sampler_step_bits_match_the_fixture(dev, family):
    """Every output of the fused CFG + sampler updates (2M, SDE at eta = 1 and eta = 0, DDIM with host and device scalars),
    byte for byte, against the digests tools/gen_sampler_step_bits.py recorded: the fixture, not the compiler, says what the
    bits of a step are (both loops of the solver kernel included: the fixture's largest case tells their roundings apart)."""
    from vd_hip import ops
    spec = importlib.util.spec_from_file_location(
        "gen_sampler_step_bits", os.path.join(os.path.dirname(GOLD), os.pardir, "tools", "gen_sampler_step_bits.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(GOLD, "sampler_step_bits.json")) as f:
        fix = json.load(f)
    assert fix["B"] == tool.B and fix["big_per"] >= 16384
    big = [c["2m"] for c in fix["solver"] if c["per"] == fix["big_per"] and c["guided"]]
    assert len(big) == 2 and all(a["x_next"] != b["x_next"] for a, b in zip(*big))      # the fixture can tell the loops apart
    for want in fix[family]:
        if family == "solver":
            got = tool.solver_case(ops, dev, want["per"], want["offset"], want["guided"])
        else:
            got = tool.ddim_case(ops, dev, want["offset"], want["guided"], want["noise"])
        assert got["inputs"] == want["inputs"], "inputs changed (torch draws differently?): %r" % (
            {k: v for k, v in want.items() if not isinstance(v, (list, dict))},)
        assert got == want


# ---- 2. order 1 == DDIM (eta = 0) ---------------------------------------------------------------------------------------

def test_order1_reproduces_ddim(tiny, dev, gold):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    net, _ = tiny
    ddim, dpm = DDIMSampler(net), DPMSolverSampler(net, order=1)
    xT = T(gold["xT"], dev)
    ct = _ci(T(gold["c_text"], dev), T(gold["u_text"], dev), 7.5)
    ci = _ci(T(gold["c_img"], dev), T(gold["u_img"], dev), 7.5, "image")
    g0 = load_gold("unet0d_tiny.npz")
    c0 = T(g0["c_img"], dev)
    x0d = torch.randn((2, 128), generator=torch.Generator().manual_seed(31)).half().to(dev)
    runs = {
        "t2i": lambda s: s.sample(steps=6, shape=[2, 4, 16, 16], x_info={"type": "image", "xt": xT}, c_info=dict(ct),
                                  verbose=False),
        "multicontext": lambda s: s.sample_multicontext(
            steps=5, shape=[2, 4, 16, 16], x_info={"type": "image", "xt": xT},
            c_info_list=[dict(ct, unconditional_guidance_scale=5.0, ratio=0.4),
                         dict(ci, unconditional_guidance_scale=5.0, ratio=0.6)], verbose=False),
        "x0_partial": lambda s: s.sample(
            steps=5, shape=[2, 4, 16, 16], x_info={"type": "image", "x0": T(gold["x0"], dev), "x0_forward_timesteps": 3,
                                                   "x0_noise": T(gold["q_noise"], dev)},
            c_info=dict(ci, unconditional_guidance_scale=1.0), verbose=False),
        "text_0d": lambda s: s.sample(steps=5, shape=[2, 128], x_info={"type": "text", "xt": x0d},
                                      c_info=_ci(c0, torch.zeros_like(c0), 4.0, "image"), verbose=False),
    }
    for name, run in runs.items():
        z_ddim, i_ddim = run(ddim)
        z_dpm, i_dpm = run(dpm)
        assert z_dpm.shape == z_ddim.shape
        assert rel_l2(z_dpm, z_ddim) < 2e-3, name
        assert rel_l2(i_dpm["pred_x0"][-1], i_ddim["pred_x0"][-1]) < 2e-3, name
        assert len(i_dpm["pred_xt"]) == len(i_ddim["pred_xt"]), name


# ---- 3. / 4. order 2 against the oracle ---------------------------------------------------------------------------------

def test_order2_tiny_vs_oracle(tiny, dev, gold):
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    from oracle import vd_oracle as O
    net, sd = tiny
    plan = O.unet_plan(**meta()["unet2d"])
    xT = torch.from_numpy(gold["xT"]).float()
    ct = _ci(torch.from_numpy(gold["c_text"]), torch.from_numpy(gold["u_text"]), 7.5)
    ci = _ci(torch.from_numpy(gold["c_img"]), torch.from_numpy(gold["u_img"]), 7.5, "image")
    on_dev = lambda c: dict(c, conditioning=c["conditioning"].half().to(dev),
                            unconditional_conditioning=c["unconditional_conditioning"].half().to(dev))
    sampler = DPMSolverSampler(net)
    z, inter = sampler.sample(steps=10, shape=[2, 4, 16, 16], x_info={"type": "image", "xt": xT.half().to(dev)},
                              c_info=on_dev(ct), verbose=False)
    assert rel_l2(z, _oracle_dpm(sd, plan, sampler, xT, [ct], 7.5)) < LATENT_TOL
    mc = [dict(ct, ratio=0.4), dict(ci, ratio=0.6)]
    z, _ = sampler.sample_multicontext(steps=10, shape=[2, 4, 16, 16], x_info={"type": "image", "xt": xT.half().to(dev)},
                                       c_info_list=[on_dev(c) for c in mc], verbose=False)
    assert rel_l2(z, _oracle_dpm(sd, plan, sampler, xT, mc, 7.5)) < LATENT_TOL


def test_order2_full_width_vs_oracle(dev):
    """Full-width UNet, 32x32 latent, B = 2, 15 guided order-2 steps (no lower-order final step at 15) vs the fp32 oracle."""
    from lib.model_zoo import get_model
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    from oracle import vd_oracle as O
    net = get_model()(full_vd_cfg(with_vae=False), verbose=False)
    sd = synth_into(net, 7)
    net = net.half()
    net.to(dev)
    g = torch.Generator().manual_seed(41)
    xT = torch.randn((2, 4, 32, 32), generator=g)
    c = torch.randn((2, 77, 768), generator=g) * 0.5
    u = torch.randn((2, 77, 768), generator=g) * 0.5
    sampler = DPMSolverSampler(net)
    z, _ = sampler.sample(steps=15, shape=[2, 4, 32, 32], x_info={"type": "image", "xt": xT.half().to(dev)},
                          c_info=_ci(c.half().to(dev), u.half().to(dev), 7.5), verbose=False)
    zref = _oracle_dpm(sd, O.unet_plan(), sampler, xT, [_ci(c, u, 7.5)], 7.5)
    err = rel_l2(z, zref)
    print("15-step DPM-Solver++(2M) rel-L2 vs fp32 oracle: %.3e" % err)
    assert err < LATENT_TOL


# ---- 5. graphs ----------------------------------------------------------------------------------------------------------

def _t2i(sampler, dev, xT, c, u, scale, steps):
    z, _ = sampler.sample(steps=steps, shape=list(xT.shape), x_info={"type": "image", "xt": xT},
                          c_info=_ci(c, u, scale), verbose=False)
    return z


def _case(dev, seed, shape=(2, 4, 16, 16)):
    g = torch.Generator().manual_seed(seed)
    xT = torch.randn(shape, generator=g).half().to(dev)
    c = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half().to(dev)
    u = (torch.randn((shape[0], 77, 128), generator=g) * 0.5).half().to(dev)
    return xT, c, u


def test_graph_replay_matches_eager(tiny, dev, monkeypatch):
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    net, _ = tiny
    xT, c, u = _case(dev, 5)
    z_graph = _t2i(DPMSolverSampler(net), dev, xT, c, u, 7.5, 8)
    monkeypatch.setenv("VD_DDIM_GRAPH", "0")
    eager = DPMSolverSampler(net)
    assert not eager.use_graph
    assert rel_l2(z_graph, _t2i(eager, dev, xT, c, u, 7.5, 8)) < 2e-3


def test_kept_graph_reused_with_other_steps_latent_and_context(tiny, dev):
    """Call 2 on the kept graph (another step count, latent, context and scale) == a fresh sampler: the history buffer is
    not read on the first step of a call, the coefficient rows and the static inputs are refreshed in place."""
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    net, _ = tiny
    shared = DPMSolverSampler(net)
    a, b = _case(dev, 6), _case(dev, 7)
    z_a = _t2i(shared, dev, *a, 7.5, 6)
    st = next(iter(shared._static.values()))
    graph = st["graph"]
    assert graph is not None and st["x0_hist"].dtype == torch.float32 and st["coef"].numel() == 8
    z_b = _t2i(shared, dev, *b, 3.0, 11)
    assert len(shared._static) == 1 and st["graph"] is graph       # replayed, not captured again
    assert rel_l2(z_b, _t2i(DPMSolverSampler(net), dev, *b, 3.0, 11)) < 5e-3
    assert rel_l2(z_a, _t2i(DPMSolverSampler(net), dev, *a, 7.5, 6)) < 5e-3
    assert rel_l2(z_a, z_b) > 0.1


def test_ddim_and_dpm_samplers_interleaved_on_one_model(tiny, dev):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    net, _ = tiny
    ddim, dpm = DDIMSampler(net), DPMSolverSampler(net)
    cases = [_case(dev, 20 + k) for k in range(2)]
    outs = []
    for k, args in enumerate(cases):
        outs.append((_t2i(ddim, dev, *args, 7.5, 5 + k), _t2i(dpm, dev, *args, 7.5, 7 + k)))
    for k, args in enumerate(cases):
        assert rel_l2(outs[k][0], _t2i(DDIMSampler(net), dev, *args, 7.5, 5 + k)) < 5e-3, k
        assert rel_l2(outs[k][1], _t2i(DPMSolverSampler(net), dev, *args, 7.5, 7 + k)) < 5e-3, k


# ---- 6. RNG / 7. sharding -----------------------------------------------------------------------------------------------

def test_rng_draws_only_the_initial_latent(tiny, dev, gold):
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    net, _ = tiny
    shape = [2, 4, 16, 16]
    torch.manual_seed(77)
    DPMSolverSampler(net).sample(steps=6, shape=shape, x_info={"type": "image"},
                                 c_info=_ci(T(gold["c_text"], dev), T(gold["u_text"], dev), 7.5), verbose=False)
    after = torch.randn(8, device=dev)
    torch.manual_seed(77)
    torch.randn(shape, device=dev, dtype=torch.float16)
    assert torch.equal(after, torch.randn(8, device=dev))


def test_sharded_world1_matches_direct_sample(tiny, dev, gold):
    from lib.model_zoo import sharded
    from lib.model_zoo.dpm_solver import DPMSolverSampler
    net, _ = tiny
    ct = _ci(T(gold["c_text"], dev), T(gold["u_text"], dev), 7.5)
    shape, seed, steps = [2, 4, 16, 16], 3, 6
    imgs = sharded.vd_sample_sharded(net, DPMSolverSampler(net), steps, shape, [dict(ct)], seed, guidance_scale=7.5,
                                     device_generator=True)
    torch.manual_seed(seed + 100)
    z, _ = DPMSolverSampler(net).sample(steps=steps, shape=shape, x_info={"type": "image"}, c_info=dict(ct), verbose=False)
    ref = net.vae_decode(z, which="image")
    assert imgs.shape == ref.shape and rel_l2(imgs, ref) < 2e-3
