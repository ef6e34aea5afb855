"""Writes tests/golden/sampler_step_bits.json: SHA-256 digests of the output bytes of the fused CFG + sampler update kernels
(ops.cfg_dpmpp_step_dev, ops.cfg_dpmpp_sde_step_dev, ops.cfg_ddim_step, ops.cfg_ddim_step_dev) on seeded inputs, so that the
bits of the sampler steps are pinned by a file and not only by two kernels agreeing with each other.

    python tools/gen_sampler_step_bits.py [--out tests/golden/sampler_step_bits.json]

Run it on the library whose bits are to be kept (VD_HIP_LIB selects a build of another commit; the ABI is the same).
tests/test_dpm_solver_gpu.py::test_sampler_step_bits_match_the_fixture imports `measure` from here and compares.

Solver cases: B = 3, two consecutive steps (a first-order row without history, then a second-order row on it; draws 0 and 1 of
the SDE entry point), views `offset` elements into larger allocations: offset 0 takes the 16-byte loop, offset 1 the scalar
loop on the same values.  The two loops round differently without noise (include/vd_hip.h), in about one fp16 output per
10^4, so the fixture must hold a case large enough to show it: the last (per, 0) / (per, 1) pair, whose `per` is raised here
until the x_next digests of the two offsets differ.  DDIM cases: n = 4099, offsets 0 / 1, guided on / off, noise on / off."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "versatile-diffusion_amd")]
os.environ.setdefault("VD_QUIET", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "sampler_step_bits.json")
B = 3
SEEDS = [11, 2 ** 35 + 5, 2 ** 63 - 1]
SMALL = [(105, 0), (4096, 0), (4096, 1)]
BIG_PER = 16384                      # where the search for the discriminating case starts
DDIM_N = 4099
DDIM_STEP = dict(a_t=0.4512, a_prev=0.5681, sqrt_one_minus_at=float(np.sqrt(1.0 - 0.4512)))
DDIM_SIGMA = 0.1375


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _view(dev, m, dtype, offset, src=None, fill=None):
    """m elements `offset` elements into a larger allocation (misaligned for offset = 1)."""
    base = torch.empty((m + offset,), device=dev, dtype=dtype)
    if fill is not None:
        base.fill_(fill)
    v = base[offset:]
    if src is not None:
        v.copy_(src)
    return v


def _tables(guided):
    from lib.model_zoo.diffusion_utils import make_ddim_timesteps
    from lib.model_zoo.dpm_solver import dpmpp_coef_table, dpmpp_sde_coef_table
    from oracle import vd_oracle as O
    ac = O.register_schedule()["alphas_cumprod"].numpy()
    ts = make_ddim_timesteps("uniform", 10, 1000, verbose=False)
    scale = 7.5 if guided else 1.0
    tabs = {"2m": dpmpp_coef_table(ac, ts, scale=scale), "sde_eta1": dpmpp_sde_coef_table(ac, ts, eta=1.0, scale=scale),
            "sde_eta0": dpmpp_sde_coef_table(ac, ts, eta=0.0, scale=scale)}
    rows = {k: (t[-1], t[5]) for k, t in tabs.items()}
    for k, (first, second) in rows.items():
        assert first[6] == 0 and second[6] != 0 and (first[7] > 0) == (k == "sde_eta1"), k
    return rows


def _solver_inputs(per, guided):
    gen = torch.Generator().manual_seed(1000 + per + 3 * guided)       # the same values at both offsets
    n = B * per
    return torch.randn(n, generator=gen).half(), torch.randn(2 * n if guided else n, generator=gen).half()


def solver_case(ops, dev, per, offset, guided):
    n = B * per
    x_h, eps_h = _solver_inputs(per, guided)
    out = {"per": per, "offset": offset, "guided": guided, "inputs": sha(torch.cat([x_h, eps_h]))}
    seeds = torch.tensor(SEEDS, dtype=torch.int64, device=dev)
    for name, rows in _tables(guided).items():
        x = _view(dev, n, torch.float16, offset, x_h).view(B, per)
        eps = _view(dev, eps_h.numel(), torch.float16, offset, eps_h)
        hist = _view(dev, n, torch.float32, offset, fill=float("nan"))     # the first step must not read it
        p0 = _view(dev, n, torch.float16, offset)
        steps = []
        for draw, row in enumerate(rows):
            coef = torch.from_numpy(np.ascontiguousarray(row)).to(dev)
            x_next = _view(dev, n, torch.float16, offset).view(B, per)
            if name == "2m":
                ops.cfg_dpmpp_step_dev(x, eps, coef, hist, guided=guided, x_next=x_next, pred_x0=p0)
            else:
                rng = torch.tensor([draw, 2], dtype=torch.int32, device=dev)
                ops.cfg_dpmpp_sde_step_dev(x, eps, coef, hist, seeds, rng, guided=guided, x_next=x_next, pred_x0=p0)
            torch.cuda.synchronize()
            steps.append({"x_next": sha(x_next), "pred_x0": sha(p0), "x0_hist": sha(hist)})
            x = x_next
        out[name] = steps
    return out


def ddim_case(ops, dev, offset, guided, noisy):
    n = DDIM_N
    gen = torch.Generator().manual_seed(2000 + 3 * guided)                # the same values at both offsets
    x_h, eps_h = torch.randn(n, generator=gen).half(), torch.randn(2 * n if guided else n, generator=gen).half()
    noise_h = torch.randn(n, generator=gen).half()
    out = {"offset": offset, "guided": guided, "noise": noisy, "inputs": sha(torch.cat([x_h, eps_h, noise_h]))}
    x, eps = _view(dev, n, torch.float16, offset, x_h), _view(dev, eps_h.numel(), torch.float16, offset, eps_h)
    noise = _view(dev, n, torch.float16, offset, noise_h) if noisy else None
    scale, sigma = (7.5 if guided else 1.0), (DDIM_SIGMA if noisy else 0.0)
    xp, p0 = ops.cfg_ddim_step(x, eps, guided=guided, guidance_scale=scale, sigma=sigma, noise=noise, **DDIM_STEP)
    torch.cuda.synchronize()
    out["host"] = {"x_prev": sha(xp), "pred_x0": sha(p0)}
    a_t, a_prev = DDIM_STEP["a_t"], DDIM_STEP["a_prev"]                   # the row DDIMSampler._coef_table would hold
    coef = torch.tensor([scale, 1.0 / np.sqrt(a_t), np.sqrt(a_prev), np.sqrt(max(1.0 - a_prev - sigma ** 2, 0.0)), sigma,
                         DDIM_STEP["sqrt_one_minus_at"]], dtype=torch.float64).float().to(dev)
    xp, p0 = _view(dev, n, torch.float16, offset), _view(dev, n, torch.float16, offset)
    ops.cfg_ddim_step_dev(x, eps, coef, guided=guided, x_prev=xp, pred_x0=p0, noise=noise)
    torch.cuda.synchronize()
    out["dev"] = {"x_prev": sha(xp), "pred_x0": sha(p0)}
    return out


def measure(ops, dev, big_per):
    """Every case of the fixture on the loaded library; `big_per` is the fixture's (or the search's) large per."""
    shapes = SMALL + [(big_per, 0), (big_per, 1)]
    return {"B": B, "big_per": big_per,
            "solver": [solver_case(ops, dev, per, off, g) for per, off in shapes for g in (True, False)],
            "ddim": [ddim_case(ops, dev, off, g, nz) for off in (0, 1) for g in (True, False) for nz in (True, False)]}


def discriminates(ops, dev, per):
    """The 2M x_next digests of the 16-byte loop (offset 0) and the scalar loop (offset 1) differ on every step, guided on
    and off: only then does the fixture tell the two roundings apart."""
    for g in (True, False):
        vec, sca = solver_case(ops, dev, per, 0, g), solver_case(ops, dev, per, 1, g)
        assert vec["inputs"] == sca["inputs"]
        if any(a["x_next"] == b["x_next"] for a, b in zip(vec["2m"], sca["2m"])):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    from vd_hip import loader, ops
    dev = torch.device("cuda:0")
    per = BIG_PER
    while not discriminates(ops, dev, per):
        per += 4096
        assert per <= 16 * BIG_PER, "the two loops never differed: is the 16-byte path taken at all?"
    fix = measure(ops, dev, per)
    big = [c for c in fix["solver"] if c["per"] == per]
    assert len(big) == 4 and all(a["x_next"] != b["x_next"] for g in (True, False)
                                 for a, b in zip(*[c["2m"] for c in big if c["guided"] == g]))
    with open(args.out, "w") as f:
        json.dump(fix, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"wrote": args.out, "big_per": per, "library": loader.lib_path(), "digest": loader.lib_digest()}))


if __name__ == "__main__":
    main()
