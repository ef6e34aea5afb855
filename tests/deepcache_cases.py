"""DeepCache in fp32 on the CPU oracle: a restatement of the cached UNet walk (the cut, the full walk that stores the deep
feature, the shallow walk that reuses it) built from oracle.vd_oracle's blocks, and DDIM / DPM-Solver++(2M) / UniPC loops on it
that follow a sampler's own coefficient table and the full / shallow schedule.  Shared by the CPU and the GPU tests."""
import numpy as np
import torch

from oracle import vd_oracle as O

FWD_TOL = 5e-3        # the project's bound on one forward against the fp32 oracle
LATENT_TOL = 1e-2     # ... and on a final latent against the fp32 oracle loop

TINY_CUTS = {1: (2, 23), 2: (5, 20), 3: (7, 16)}
FULL_CUTS = {1: (2, 66), 2: (5, 63), 3: (8, 60), 4: (10, 56), 5: (13, 53)}


def flat_order(plan):
    return plan["i_order"] + plan["m_order"] + plan["o_order"]


def cut(order, k):
    """(a, b): order[0:a] ends with the k-th save, order[b:] begins with the k-th load from the end."""
    S = [i for i, s in enumerate(order) if s == "save_hidden_feature"]
    L = [i for i, s in enumerate(order) if s == "load_hidden_feature"]
    n = len(S)
    assert len(L) == n and 1 <= k <= n - 1
    return S[k - 1] + 1, L[n - k]


def full_steps(total, interval):
    return [i for i in range(total) if i % interval == 0]


def walk(sd, plan, x, t, contexts, depth=None, cache=None, mode="full", x_type="image"):
    """The UNet on x [B, C, H, W] at timesteps t with contexts [(type, c, ratio), ...].  depth None: the plain walk.
    mode "full": the whole walk, with a copy of the tensor in front of the cut's load kept in cache["f"]; "shallow": the prefix for
    its skips, cache["f"] in place of everything up to the cut, the suffix."""
    order = flat_order(plan)
    emb = O.time_embed(sd, "diffuser.%s.time_embed" % x_type, O.timestep_embedding(t, plan["model_channels"]))
    ratios = np.array([float(r) for _, _, r in contexts])
    ratios = ratios / ratios.sum()
    kinds, di, ci = [], 0, 0
    for s in order:
        if s == "d":
            kinds.append(("d", di))
            di += 1
        elif s == "c":
            kinds.append(("c", ci))
            ci += 1
        else:
            kinds.append((s, None))
    hs = []

    def run(lo, hi, h):
        for s, j in kinds[lo:hi]:
            if s == "d":
                h = O._data_block(sd, "diffuser.%s.data_blocks.%d" % (x_type, j), plan["data"][j][0], h, emb)
            elif s == "c":
                out = None
                for (ct, c, _), r in zip(contexts, ratios):
                    hi_ = O.spatial_transformer(sd, "diffuser.%s.context_blocks.%d.0" % (ct, j), h, c, plan["ctx"][j][1])
                    if len(contexts) > 1:
                        hi_ = hi_ * float(r)
                    out = hi_ if out is None else out + hi_
                h = out
            elif s == "save_hidden_feature":
                hs.append(h)
            else:
                h = torch.cat([h, hs.pop()], 1)
        return h

    with torch.no_grad():
        if depth is None:
            return run(0, len(kinds), x)
        a, b = cut(order, depth)
        if mode == "full":
            h = run(0, b, x)
            cache["f"] = h.clone()
            return run(b, len(kinds), h)
        assert mode == "shallow"
        run(0, a, x)
        return run(b, len(kinds), cache["f"])


def cfg_contexts(contexts, guided):
    """[(type, c, ratio)] of sampler-style context dicts on the CPU in fp32; guided: the batch [uncond ; cond]."""
    return [(c["type"], (torch.cat([c["unconditional_conditioning"], c["conditioning"]]) if guided else c["conditioning"]).float().cpu(),
             c.get("ratio", 1.0)) for c in contexts]


def oracle_loop(sd, plan, sampler, kind, xT, contexts, scale, interval=1, depth=1):
    """The loop `sampler` ran last ("ddim", "2m" or "unipc"), in fp32 on the oracle, driven by the sampler's own coefficient
    table; step k in sampling order is a full walk iff k % interval == 0, else a shallow walk on the kept feature."""
    ts = sampler.ddim_timesteps
    S = len(ts)
    tab = sampler._coef_table(S, scale, torch.device("cpu")).double().numpy()
    guided = scale != 1.0
    cs = cfg_contexts(contexts, guided)
    x = xT.float().cpu()
    cache = {}
    hist = xl = m1 = m2 = m3 = None
    for k, i in enumerate(reversed(range(S))):
        r = [float(v) for v in tab[i]]
        xin = torch.cat([x, x]) if guided else x
        t = torch.full((xin.shape[0],), int(ts[i]), dtype=torch.long)
        if interval == 1:
            eps = walk(sd, plan, xin, t, cs)
        else:
            eps = walk(sd, plan, xin, t, cs, depth=depth, cache=cache, mode="full" if k % interval == 0 else "shallow")
        if guided:
            e_u, e_c = eps.chunk(2)
            e = e_u + r[0] * (e_c - e_u)
        else:
            e = eps
        if kind == "ddim":      # {scale, 1/sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev - sigma^2), sigma, sqrt(1 - a_t)}
            p0 = (x - r[5] * e) * r[1]
            x = r[2] * p0 + r[3] * e
        elif kind == "2m":      # {scale, 1/sqrt(a_t), sqrt(1 - a_t), sigma_next/sigma_t, c_d, w_cur, w_prev, 0}
            p0 = (x - r[2] * e) * r[1]
            d = r[5] * p0 + (r[6] * hist if r[6] != 0 else 0.0)
            x, hist = r[3] * x + r[4] * d, p0
        else:                   # the row layout of unipc.unipc_coef_table
            assert kind == "unipc"
            mt = (x - r[2] * e) * r[1]
            xc = x
            if r[3] != 0:
                xc = r[4] * xl + r[8] * mt
                for c, m in ((r[5], m1), (r[6], m2), (r[7], m3)):
                    if c != 0:
                        xc = xc + c * m
            xn = r[9] * xc + r[10] * mt
            for c, m in ((r[11], m1), (r[12], m2)):
                if c != 0:
                    xn = xn + c * m
            xl, m1, m2, m3, x = xc, mt, m1, m2, xn
    return x
