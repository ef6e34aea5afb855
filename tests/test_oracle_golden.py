"""The oracle (oracle/vd_oracle.py) against fixtures produced by the reference itself (oracle/gen_golden.py).

CPU only.  fp32 vs fp32, so tolerances are tight: 1e-5 relative L2 (different op order only); the DDIM index
schedule and the schedule buffers must be bit-exact.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import synth, vd_oracle as O
from vdtest_util import fullwidth_inputs, live_case_inputs, load_ref_json, published_vocab_files, random_tokenizer_texts

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return {k: v for k, v in np.load(os.path.join(GOLD, name), allow_pickle=False).items()}


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLD, "meta.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tiny_sd(meta):
    g = load("unet_tiny.npz")
    shapes = {str(k): tuple(json.loads(str(s))) for k, s in zip(g["state_keys"], g["state_shapes"])}
    sd = synth.synth_state_dict(shapes, meta["seed"])
    sd.update(O.register_schedule())
    return sd


def test_schedule_bit_exact():
    g = load("schedule.npz")
    s = O.register_schedule()
    for k, v in s.items():
        assert np.array_equal(v.numpy(), g[k]), k
    # known answers quoted in SURVEY.md 8c
    assert s["betas"][0].item() == pytest.approx(0.00085, abs=1e-9)
    assert s["alphas_cumprod"][999].item() == np.float32(0.004660098347812891)
    for steps in (50, 10, 5, 4):
        d = O.ddim_schedule(s["alphas_cumprod"], steps, 0.0)
        assert np.array_equal(d["timesteps"], g["ddim%d_timesteps" % steps])
        assert np.array_equal(d["alphas"].numpy(), g["ddim%d_alphas" % steps])
        assert np.array_equal(np.asarray(d["alphas_prev"]), g["ddim%d_alphas_prev" % steps])
        assert np.array_equal(d["sigmas"].numpy(), g["ddim%d_sigmas" % steps])
        assert np.array_equal(d["sqrt_one_minus_alphas"].numpy(), g["ddim%d_sqrt_one_minus_alphas" % steps])
    assert np.array_equal(O.make_ddim_timesteps(50), 1 + 20 * np.arange(50))
    assert np.array_equal(O.make_ddim_timesteps(10), 1 + 100 * np.arange(10))
    d = O.ddim_schedule(s["alphas_cumprod"], 10, 0.7)
    assert np.allclose(d["sigmas"].numpy(), g["ddim10_eta07_sigmas"], rtol=1e-6, atol=0)
    with pytest.raises(IndexError):  # reference quirk: S=3 indexes alphas_cumprod[1000]
        O.ddim_schedule(s["alphas_cumprod"], 3, 0.0)


def test_timestep_embedding():
    g = load("schedule.npz")
    t = T(g["temb_t"])
    assert np.array_equal(O.timestep_embedding(t, 320).numpy(), g["temb_320"])
    assert np.array_equal(O.timestep_embedding(t, 64).numpy(), g["temb_64"])
    e = O.timestep_embedding(torch.tensor([981]), 320)[0]
    assert np.allclose(e[:3].numpy(), [0.67995721, -0.79842919, 0.57806414], atol=1e-6)
    assert np.allclose(e[160:163].numpy(), [0.73325181, 0.60208869, 0.81599128], atol=1e-6)


def test_unet_plan_matches_reference_structure(meta):
    """Appendix A of SURVEY.md: the full-size 2D UNet has 30 data / 16 context blocks and 12 skips."""
    p = O.unet_plan()
    assert len(p["data"]) == 30 and len(p["ctx"]) == 16
    assert p["i_order"].count("save_hidden_feature") == 12 and p["o_order"].count("load_hidden_feature") == 12
    assert p["m_order"] == ["d", "c", "d"]
    assert [c for c, _ in p["ctx"]] == [320, 320, 640, 640, 1280, 1280, 1280, 1280, 1280, 1280, 640, 640, 640, 320, 320, 320]
    assert p["data"][14] == ("res", 2560, 1280) and p["data"][20] == ("res", 1920, 1280) and p["data"][26] == ("res", 960, 320)
    tiny = O.unet_plan(**meta["unet2d"])
    assert [h for _, h in tiny["ctx"]] == [1, 2, 2, 2, 2, 1, 1]


def test_unet_tiny_forward(meta, tiny_sd):
    g = load("unet_tiny.npz")
    plan = O.unet_plan(**meta["unet2d"])
    x, t = T(g["x"]), T(g["t"])
    with torch.no_grad():
        e_text = O.apply_model(tiny_sd, plan, x, t, T(g["c_text"]), c_type="text", global_ptr="image")
        e_img = O.apply_model(tiny_sd, plan, x, t, T(g["c_img"]), c_type="image", global_ptr="image")
        e_mix = O.apply_model_multicontext(tiny_sd, plan, x, t, [("text", T(g["c_text"]), 0.4), ("image", T(g["c_img"]), 0.6)])
    assert rel(e_text, g["eps_text"]) < 1e-5
    assert rel(e_img, g["eps_image"]) < 1e-5
    assert rel(e_mix, g["eps_mix"]) < 1e-5
    assert float(np.abs(g["eps_text"]).mean()) > 1e-2  # the synthetic weights do not zero the output


def test_unet0d_tiny_forward(meta, tiny_sd):
    """Text-latent (0-D) data flow: FCBlock_MultiDim / Linear_MultiDim data blocks of diffuser['text'] with
    image- or text-typed context blocks, time_embed through the global pointer."""
    g = load("unet0d_tiny.npz")
    plan = O.unet0d_plan(**meta["unet0d"])
    full = O.unet0d_plan()
    assert len(full["data"]) == 30 and len(full["ctx"]) == 16 and full["i_order"] == O.unet_plan()["i_order"]
    x, t = T(g["x"]), T(g["t"])
    with torch.no_grad():
        e_img = O.apply_model(tiny_sd, plan, x, t, T(g["c_img"]), x_type="text", c_type="image", global_ptr="image")
        e_text = O.apply_model(tiny_sd, plan, x, t, T(g["c_text"]), x_type="text", c_type="text", global_ptr="image")
    assert e_img.shape == (2, 128)
    assert rel(e_img, g["eps_image"]) < 1e-5
    assert rel(e_text, g["eps_text"]) < 1e-5
    assert float(np.abs(g["eps_image"]).mean()) > 1e-2


def test_ddim_tiny(meta, tiny_sd):
    g = load("ddim_tiny.npz")
    plan = O.unet_plan(**meta["unet2d"])
    ac = tiny_sd["alphas_cumprod"]
    ctx_t = {"type": "text", "conditioning": T(g["c_text"]), "unconditional_conditioning": T(g["u_text"])}
    ctx_i = {"type": "image", "conditioning": T(g["c_img"]), "unconditional_conditioning": T(g["u_img"])}
    with torch.no_grad():
        z, p0 = O.ddim_sample(tiny_sd, plan, ac, T(g["xT"]), [ctx_t], 5, 7.5, global_ptr="image")
        assert rel(z, g["z_t2i"]) < 1e-4 and rel(p0, g["pred_x0_t2i"]) < 1e-4
        zm, _ = O.ddim_sample(tiny_sd, plan, ac, T(g["xT"]), [dict(ctx_t, ratio=0.4), dict(ctx_i, ratio=0.6)], 4, 5.0)
        assert rel(zm, g["z_mc"]) < 1e-4
        sched = O.ddim_schedule(ac, 5)
        ts = torch.full((2,), int(sched["timesteps"][3]), dtype=torch.long)
        x_start = O.q_sample(tiny_sd, T(g["x0"]), ts, T(g["q_noise"]))
        zi, _ = O.ddim_sample(tiny_sd, plan, ac, x_start, [ctx_i], 5, 1.0, forward_steps=3, global_ptr="image")
        assert rel(zi, g["z_i2i"]) < 1e-4


def test_vae_tiny(meta, tiny_sd):
    g = load("vae_tiny.npz")
    dd = meta["vae"]["ddconfig"]
    kw = dict(ch_mult=dd["ch_mult"], num_res_blocks=dd["num_res_blocks"])
    with torch.no_grad():
        mom = O.vae_encode_moments(tiny_sd, "vae.image", T(g["img"]), **kw)
        assert rel(mom, g["moments"]) < 1e-5
        z = O.diag_gaussian_sample(mom, T(g["post_noise"])) * 0.18215
        assert rel(z, g["z"]) < 1e-5
        dec = O.vae_decode(tiny_sd, "vae.image", T(g["z"]) / 0.18215, **kw)
        assert rel(dec, g["dec"]) < 1e-5
        dec2 = O.vae_decode(tiny_sd, "vae.image", T(g["zlat"]) * (1.0 / 0.18215), **kw)
        assert rel(dec2, g["dec2"]) < 1e-5


def test_clip_tiny(meta):
    from transformers import CLIPConfig, CLIPModel
    g = load("clip_tiny.npz")
    cfg = meta["clip"]
    shapes = synth.shapes_of(CLIPModel(CLIPConfig(**cfg)))
    sd = synth.synth_state_dict({"ctx.text.model." + k: v for k, v in shapes.items()}, meta["seed"])
    tc, vc = cfg["text_config"], cfg["vision_config"]
    ids = T(g["input_ids"])
    px = torch.randn((3, 3, 224, 224), generator=torch.Generator().manual_seed(int(g["px_seed"])))
    with torch.no_grad():
        zt = O.clip_text_context(sd, "ctx.text.model", ids, tc["num_attention_heads"], tc["num_hidden_layers"])
        assert rel(zt, g["z_text"]) < 1e-5
        zi = O.clip_image_context(sd, "ctx.text.model", px, vc["num_attention_heads"], vc["num_hidden_layers"])
        assert rel(zi, g["z_img"]) < 1e-5
        vt, all_ones = O.clip_vtoken_mask(T(g["masks"]))
        assert not all_ones
        zm = O.clip_image_context(sd, "ctx.text.model", px, vc["num_attention_heads"], vc["num_hidden_layers"], vtoken_mask=vt)
        assert rel(zm, g["z_img_masked"]) < 1e-5


def test_adjust_rank_oracle_vs_reference_fixture():
    """oracle/adjust_rank.py (restatement of app.py:48-127) against tests/golden/adjust_rank.npz, which the REFERENCE's own
    source lines produced (oracle/gen_golden_adjust_rank.py).  pca_lowrank is randomised: another seed must land on the
    same reconstruction; the exact-SVD limit the device kernel computes agrees to fp16 output rounding."""
    from oracle import adjust_rank as A
    g = load("adjust_rank.npz")
    x = torch.from_numpy(g["x"])
    for lvl, key in ((0.0, "y_00"), (0.3, "y_03"), (0.8, "y_08"), (1.0, "y_10")):
        torch.manual_seed(99)
        assert rel(A.adjust_rank(x.clone(), lvl), g[key]) < 1e-4, lvl
        assert rel(A.exact(x.float(), lvl), g[key]) < 5e-4, lvl
    assert A.adjust_rank(x, 0.5) is x
    # the product's host-side level curves are the reference's
    from lib.app_ops import adjust_rank
    ar = adjust_rank(max_drop_rank=[1, 5], q=20)
    for lvl in (0.0, 0.1, 0.3, 0.49, 0.51, 0.8, 1.0):
        f, keep = ar.scales(lvl)
        fo, ko = A.level_scales(lvl)
        assert keep == ko and np.allclose(f, fo, rtol=0, atol=1e-12), lvl


def _optimus_sd():
    meta_o = json.load(open(os.path.join(GOLD, "optimus_tokenizer.json")))
    cfg, seed = meta_o["config"], meta_o["seed"]
    from lib.model_zoo.optimus import optimus_gpt2_connector
    net = optimus_gpt2_connector(cfg, latent_size=cfg["latent_size"])
    shapes = {"decoder." + k: v for k, v in synth.shapes_of(net).items()}
    sd = synth.synth_state_dict(shapes, seed)
    sd["decoder.lm_head.weight"] = sd["decoder.transformer.wte.weight"]     # tie_weights
    return meta_o, cfg, net, sd


def test_optimus_gpt2_oracle_vs_reference_fixture():
    """oracle/optimus_oracle.py (GPT-2 decoder with the latent as embedding + per-layer memory, and the sampling loop)
    against outputs of the REFERENCE's vendored GPT2ForLatentConnector_XX (oracle/gen_golden_optimus.py); the product
    module's state-dict key layout equals the reference module's (same synthetic-weight names were used there)."""
    from oracle import optimus_oracle as OO
    meta_o, cfg, net, sd = _optimus_sd()
    g = load("optimus_tiny.npz")
    lg = OO.gpt2_logits(sd, "decoder", T(g["ids"]), T(g["z"]), cfg["n_head"], cfg["n_layer"])
    assert rel(lg, g["logits"]) < 1e-5
    torch.manual_seed(99)
    seq = OO.sample_sequence(sd, "decoder", T(g["z"])[0], 5, 7, cfg["n_head"], cfg["n_layer"], max_length=12)
    assert seq.tolist() == g["sampled"].tolist()
    # reference state-dict names: every tensor the reference module holds exists here with the same shape
    expect = {"transformer.wte.weight", "transformer.wpe.weight", "transformer.h.0.attn.bias", "transformer.h.1.mlp.c_proj.weight",
              "transformer.linear.weight", "transformer.linear_emb.weight", "transformer.ln_f.bias", "lm_head.weight"}
    assert expect <= set(net.state_dict())
    assert net.state_dict()["transformer.h.0.attn.c_attn.weight"].shape == (cfg["n_embd"], 3 * cfg["n_embd"])
    assert net.lm_head.weight is net.transformer.wte.weight


def test_gpt2_tokenizer_matches_reference(tmp_path):
    """The product's GPT-2 byte-level BPE (lib/model_zoo/optimus.py) against ids / decoded strings the reference's
    vendored tokenizer produced (tests/golden/optimus_tokenizer.json), with the published vocabulary and merges restricted
    to the entries those strings use (vdtest_util.published_vocab_files)."""
    from lib.model_zoo.optimus import optimus_gpt2_tokenizer
    tk = json.load(open(os.path.join(GOLD, "optimus_tokenizer.json")))["tokenizer"]
    vocab, merges, _ = published_vocab_files(tmp_path)
    tok = optimus_gpt2_tokenizer(vocab_file=vocab, merges_file=merges)
    tok.add_special_tokens({"pad_token": "<PAD>", "bos_token": "<BOS>", "eos_token": "<EOS>"})
    assert [tok.encode("<BOS>"), tok.encode("<EOS>"), tok.encode("<PAD>")] == tk["special"] and len(tok) == tk["len"]
    for c in tk["cases"]:
        ids = tok.encode("<BOS>") + tok.encode(c["text"]) + tok.encode("<EOS>")
        assert ids == c["ids"], c["text"]
        assert tok.decode(ids, clean_up_tokenization_spaces=True) == c["decoded"]
    assert tok.encode("<BOS> hello <EOS>") == tok.encode("<BOS>") + tok.encode("hello") + tok.encode("<EOS>")


# ---- Optimus encode side (BERT) -----------------------------------------------------------------------------------------
def _bert_meta():
    return json.load(open(os.path.join(GOLD, "optimus_bert_tokenizer.json")))


def reduced_bert_vocab(path):
    """A vocabulary file holding exactly the pieces the golden cases use, at their published ids (every other line a
    placeholder): greedy longest-match over a subset that contains the full vocabulary's matches finds the same pieces,
    so the fixture texts tokenise identically without the 213 KB published file."""
    m = _bert_meta()
    tk = m["tokenizer"]
    lines = ["[unused-%d]" % i for i in range(tk["len"])]
    cls_id, sep_id, pad_id, unk_id = tk["special"]
    lines[cls_id], lines[sep_id], lines[pad_id], lines[unk_id], lines[103] = "[CLS]", "[SEP]", "[PAD]", "[UNK]", "[MASK]"
    for c in tk["cases"]:
        for piece, i in zip(c["pieces"], c["ids"]):
            lines[i] = piece
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return path


def test_bert_oracle_vs_reference_fixture():
    """oracle/optimus_oracle.py bert_forward / bert_latent_mu against outputs of the REFERENCE's vendored
    BertForLatentConnector_XX on right-padded batches (oracle/gen_golden_optimus_bert.py), and the product module's
    state-dict key layout against the reference's (the synthetic weights are addressed by those names)."""
    from lib.model_zoo.optimus import optimus_bert_connector
    from oracle import optimus_oracle as OO
    m = _bert_meta()
    cfg = m["config"]
    net = optimus_bert_connector(cfg, latent_size=cfg["latent_size"])
    sd = synth.synth_state_dict({"encoder." + k: v for k, v in synth.shapes_of(net).items()}, m["seed"])
    g = load("optimus_bert_tiny.npz")
    ids = T(g["ids"]).long()
    seq, pooled = OO.bert_forward(sd, "encoder", ids, (ids > 0).float(), cfg["num_attention_heads"], cfg["num_hidden_layers"])
    assert rel(seq, g["seq"]) < 1e-5 and rel(pooled, g["pooled"]) < 1e-5
    assert rel(OO.bert_latent_mu(sd, "encoder", pooled), g["mu"]) < 1e-5
    keys = set(net.state_dict())
    assert {"embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
            "embeddings.LayerNorm.bias", "encoder.layer.1.attention.self.query.weight", "encoder.layer.0.attention.output.dense.bias",
            "encoder.layer.0.attention.output.LayerNorm.weight", "encoder.layer.1.intermediate.dense.weight",
            "encoder.layer.1.output.dense.weight", "encoder.layer.1.output.LayerNorm.bias", "pooler.dense.weight", "linear.weight"} <= keys
    assert len(keys) == 5 + 16 * cfg["num_hidden_layers"] + 2 + 1
    assert net.linear.weight.shape == (2 * cfg["latent_size"], cfg["hidden_size"])


@pytest.mark.parametrize("full", [False, True])
def test_bert_tokenizer_matches_reference(full, tmp_path):
    """The product's BERT basic + WordPiece tokenizer against pieces / ids the reference's vendored BertTokenizer produced
    (cased and lower-casing variants, accents, CJK, punctuation runs, an over-long word, a special token inside the text);
    with the published vocabulary restricted to the pieces of every tokenizer fixture (vdtest_util.published_vocab_files,
    cased and lower-casing cases), and with the reduced one built from the cased cases alone."""
    from lib.model_zoo.optimus import optimus_bert_tokenizer
    vocab = published_vocab_files(tmp_path)[2] if full else reduced_bert_vocab(str(tmp_path / "vocab.txt"))
    tk = _bert_meta()["tokenizer"]
    tok = optimus_bert_tokenizer(vocab_file=vocab, do_lower_case=False, max_len=512)
    assert [tok.cls_token_id, tok.sep_token_id, tok.pad_token_id, tok.unk_token_id] == tk["special"] and len(tok) == tk["len"]
    assert tok.add_special_tokens_single_sentence([5, 6]) == tk["with_special"]
    for c in tk["cases"]:
        assert tok.tokenize(c["text"]) == c["pieces"], c["text"]
        assert [tok._convert_token_to_id(p) for p in c["pieces"]] == c["ids"]
    if full:
        lc = optimus_bert_tokenizer(vocab_file=vocab, do_lower_case=True, max_len=512)
        for c in tk["cases_lower"]:
            assert lc.tokenize(c["text"]) == c["pieces"], c["text"]
    assert tok.tokenize("   ") == [] and tok.tokenize("") == []
    with pytest.raises(FileNotFoundError):
        optimus_bert_tokenizer(vocab_file="/nonexistent/vocab.txt").tokenize("a")


@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (5, 1.0), (0, 0.9), (0, 0.3), (40, 0.8), (1, 0.5), (1000, 0.99)])
def test_top_k_top_p_filter_equals_reference_rule(top_k, top_p):
    """The product filters the PROBABILITY vector (lib/model_zoo/optimus.top_k_top_p_filtering) where the reference
    filters logits (optimus.py:690-721): the sampling distribution softmax(filtered logits) must be the same."""
    from lib.model_zoo.optimus import top_k_top_p_filtering as mine
    from oracle import optimus_oracle as OO
    g = torch.Generator().manual_seed(top_k * 7 + int(top_p * 100))
    for temperature in (1.0, 0.7):
        logits = torch.randn(300, generator=g) * 3.0 / temperature
        ref = torch.softmax(OO.top_k_top_p_filtering(logits, top_k=top_k, top_p=top_p), dim=-1)
        p = mine(torch.softmax(logits, dim=-1), top_k=top_k, top_p=top_p)
        p = p / p.sum()
        if top_p >= 1.0:   # the reference's `cumulative > 1.0` fires on fp32 round-off in the far tail only: the product skips it
            differ = (p > 0) != (ref > 0)
            assert float(p[differ].sum()) < 1e-5 and torch.allclose(p, ref, rtol=0, atol=1e-6)
            continue
        assert torch.equal(p > 0, ref > 0)
        assert torch.allclose(p, ref, rtol=1e-5, atol=1e-8)


def test_tokenizers_against_live_reference_on_random_strings(tmp_path):
    """300 seeded random strings (ASCII words, digits, punctuation runs, accents, CJK, emoji, odd whitespace, control
    characters, contractions) through the REFERENCE's own BERT and GPT-2 tokenizers (oracle/ref_tokenize.py, stored in
    tests/golden/ref_tokenize.json.gz) and through the product's re-implementations: identical pieces / ids / decoded text."""
    from lib.model_zoo.optimus import optimus_bert_tokenizer, optimus_gpt2_tokenizer
    texts = random_tokenizer_texts()
    ref = load_ref_json("ref_tokenize.json.gz")
    assert ref["texts"] == texts
    gv, gm, bv = published_vocab_files(tmp_path)
    bert = optimus_bert_tokenizer(vocab_file=bv, do_lower_case=False, max_len=512)
    gpt2 = optimus_gpt2_tokenizer(vocab_file=gv, merges_file=gm)
    gpt2.add_special_tokens({"pad_token": "<PAD>", "bos_token": "<BOS>", "eos_token": "<EOS>"})
    bad = []
    for i, t in enumerate(texts):
        if bert.tokenize(t) != ref["bert"][i]:
            bad.append(("bert", t, bert.tokenize(t), ref["bert"][i]))
        ids = gpt2.encode(t)
        if ids != ref["gpt2"][i]:
            bad.append(("gpt2", t, ids, ref["gpt2"][i]))
        elif gpt2.decode(ids, clean_up_tokenization_spaces=True) != ref["gpt2_decoded"][i]:
            bad.append(("gpt2-decode", t, gpt2.decode(ids, clean_up_tokenization_spaces=True), ref["gpt2_decoded"][i]))
    assert not bad, bad[:3]


def test_oracle_against_live_reference_on_random_cases(tiny_sd, meta):
    """Beyond the fixed fixtures: 8 seeded random cases (batch 1-3, 8/16/24-pixel ragged latents, context lengths 3-89,
    random timesteps, mixing ratios, guidance scales, step counts; single-context, two-context and partial-schedule DDIM
    loops; KL-f8 encode / decode at random image sizes; the text-latent flow) run through the LIVE reference (oracle/ref_live_cases.py, seed 20260924, stored in
    tests/golden/ref_live_cases.npz, inputs drawn again from the seeds) and replayed through the oracle: forwards < 1e-5, final
    latents < 1e-4 rel-L2."""
    d = np.load(os.path.join(GOLD, "ref_live_cases.npz"))
    plan = O.unet_plan(**meta["unet2d"])
    flavours = set()
    for k in range(int(d["n"])):
        inp = live_case_inputs(d, k)
        g = lambda n: inp[n] if n in inp else T(d["%d_%s" % (k, n)])
        ratio, steps, scale, flavour, fwd = [float(v) for v in d["%d_meta" % k]]
        x, t, ct, ci = g("x"), g("t").long(), g("ct"), g("ci")
        with torch.no_grad():
            assert rel(O.apply_model(tiny_sd, plan, x, t, ct, c_type="text", global_ptr="image"), g("e_t")) < 1e-5, k
            assert rel(O.apply_model(tiny_sd, plan, x, t, ci, c_type="image", global_ptr="image"), g("e_i")) < 1e-5, k
            mix = O.apply_model_multicontext(tiny_sd, plan, x, t, [("text", ct, ratio), ("image", ci, 1.0 - ratio)], global_ptr="image")
            assert rel(mix, g("e_m")) < 1e-5, k
            c_text = {"type": "text", "conditioning": ct, "unconditional_conditioning": g("ut"), "ratio": ratio}
            c_img = {"type": "image", "conditioning": ci, "unconditional_conditioning": torch.zeros_like(ci), "ratio": 1.0 - ratio}
            flavours.add(int(flavour))
            if int(flavour) == 0:
                z, _ = O.ddim_sample(tiny_sd, plan, tiny_sd["alphas_cumprod"], g("xT"), [dict(c_text, ratio=1.0)], int(steps), scale,
                                     global_ptr="image")
            elif int(flavour) == 1:
                z, _ = O.ddim_sample(tiny_sd, plan, tiny_sd["alphas_cumprod"], g("xT"), [c_text, c_img], int(steps), scale,
                                     global_ptr="image")
            else:
                sched = O.ddim_schedule(tiny_sd["alphas_cumprod"], int(steps), 0.0)
                tq = torch.full((x.shape[0],), int(sched["timesteps"][int(fwd)]), dtype=torch.long)
                x_start = O.q_sample(tiny_sd, x, tq, g("xT"))
                z, _ = O.ddim_sample(tiny_sd, plan, tiny_sd["alphas_cumprod"], x_start, [dict(c_img, ratio=1.0)], int(steps), scale,
                                     global_ptr="image", forward_steps=int(fwd))
            assert rel(z, g("z")) < 1e-4, (k, flavour)
            dd = meta["vae"]["ddconfig"]
            kw = dict(ch_mult=dd["ch_mult"], num_res_blocks=dd["num_res_blocks"])
            assert rel(O.vae_encode_moments(tiny_sd, "vae.image", g("img"), **kw), g("mom")) < 1e-5, k
            assert rel(O.vae_decode(tiny_sd, "vae.image", g("zl") * (1.0 / 0.18215), **kw), g("dec")) < 1e-5, k
            p0d = O.unet0d_plan(**meta["unet0d"])
            assert rel(O.apply_model(tiny_sd, p0d, g("x0d"), t, ci, x_type="text", c_type="image", global_ptr="image"), g("e0_i")) < 1e-5, k
            assert rel(O.apply_model(tiny_sd, p0d, g("x0d"), t, ct, x_type="text", c_type="text", global_ptr="image"), g("e0_t")) < 1e-5, k
    assert flavours == {0, 1, 2}


def test_oracle_against_live_reference_at_full_width():
    """The oracle pinned at the width the GPU parity tests use it at: VD_v2_0 built by the REFERENCE's registry from its own
    YAML configs (openai_unet_2d_v1, 859.5 M parameters; openai_unet_0d_v1_dc, 1.71 B), synthetic weights regenerated by
    name on both sides, 16x16 latent, L = 77 text / 257 image tokens (oracle/ref_live_fullwidth.py, seed 7, stored in
    tests/golden/ref_live_fullwidth.npz, inputs drawn again from the seeds):
    single-context and mixed-context forwards of the image flow, the text-latent (0-D) flow with either context, and a
    4-step guided DDIM loop replayed through the oracle: forwards < 2e-5, final latent < 1e-4 rel-L2."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seed = 7
    d = np.load(os.path.join(GOLD, "ref_live_fullwidth.npz"))
    assert [int(v) for v in d["nparams"]] == [859520964, 1706797888]
    sys.path.insert(0, os.path.join(root, "versatile-diffusion_amd"))
    from lib.cfg_helper import CfgDict, model_cfg_bank
    from lib.model_zoo import get_model
    bank = model_cfg_bank()
    cfg = CfgDict(type="vd_v2_0", args=CfgDict(
        vae_cfg_list=[], ctx_cfg_list=[["image", "ctx-image-placeholder"], ["text", "ctx-text-placeholder"]],
        diffuser_cfg_list=[["image", bank("openai_unet_2d_v1")], ["text", bank("openai_unet_0d_v1_dc")]],
        global_layer_ptr="image", latent_scale_factor={"image": 0.18215}, beta_linear_start=0.00085,
        beta_linear_end=0.012, timesteps=1000, use_ema=False))
    with torch.device("meta"):       # key names and shapes only (this package's modules mirror the reference's layout)
        shapes = synth.shapes_of(get_model()(cfg, verbose=False))
    sd = synth.synth_state_dict(shapes, seed)
    sd.update(O.register_schedule())
    inp = fullwidth_inputs()
    g = lambda n: inp[n] if n in inp else T(d[n])
    x, t, ct, ci, x0d = g("x"), g("t").long(), g("ct"), g("ci"), g("x0d")
    p2, p0 = O.unet_plan(**dict(bank("openai_unet_2d_v1").args)), O.unet0d_plan(**dict(bank("openai_unet_0d_v1_dc").args))
    with torch.no_grad():
        assert rel(O.apply_model(sd, p2, x, t, ct, c_type="text", global_ptr="image"), g("e_t")) < 2e-5
        assert rel(O.apply_model(sd, p2, x, t, ci, c_type="image", global_ptr="image"), g("e_i")) < 2e-5
        mix = O.apply_model_multicontext(sd, p2, x, t, [("text", ct, 0.4), ("image", ci, 0.6)], global_ptr="image")
        assert rel(mix, g("e_m")) < 2e-5
        assert rel(O.apply_model(sd, p0, x0d, t, ct, x_type="text", c_type="text", global_ptr="image"), g("e0_t")) < 2e-5
        assert rel(O.apply_model(sd, p0, x0d, t, ci, x_type="text", c_type="image", global_ptr="image"), g("e0_i")) < 2e-5
        c_text = {"type": "text", "conditioning": ct, "unconditional_conditioning": g("ut"), "ratio": 1.0}
        z, _ = O.ddim_sample(sd, p2, sd["alphas_cumprod"], g("xT"), [c_text], 4, 7.5, global_ptr="image")
        assert rel(z, g("z")) < 1e-4


def test_optimus_oracle_against_live_reference_on_random_cases():
    """GPT-2 latent-connector logits (random sequence lengths 1-19, batches 1-3) and BERT latent-connector outputs (random
    right-padded batches, lengths 2-29, incl. rows without padding) from the LIVE reference classes
    (oracle/ref_live_optimus.py, seed 31, 6 cases, stored in tests/golden/ref_live_optimus.npz) against oracle/optimus_oracle.py."""
    from oracle import optimus_oracle as OO
    d = np.load(os.path.join(GOLD, "ref_live_optimus.npz"))
    meta_o, cfg, net, sd = _optimus_sd()
    mb = _bert_meta()
    from lib.model_zoo.optimus import optimus_bert_connector
    bnet = optimus_bert_connector(mb["config"], latent_size=mb["config"]["latent_size"])
    bsd = synth.synth_state_dict({"encoder." + k: v for k, v in synth.shapes_of(bnet).items()}, mb["seed"])
    for k in range(int(d["n"])):
        lg = OO.gpt2_logits(sd, "decoder", T(d["%d_gpt_ids" % k]).long(), T(d["%d_gpt_z" % k]), cfg["n_head"], cfg["n_layer"])
        assert rel(lg, d["%d_gpt_logits" % k]) < 1e-5, k
        ids = T(d["%d_bert_ids" % k]).long()
        seq, pooled = OO.bert_forward(bsd, "encoder", ids, (ids > 0).float(), mb["config"]["num_attention_heads"],
                                      mb["config"]["num_hidden_layers"])
        assert rel(seq, d["%d_bert_seq" % k]) < 1e-5 and rel(pooled, d["%d_bert_pooled" % k]) < 1e-5, k
        assert rel(OO.bert_latent_mu(bsd, "encoder", pooled), d["%d_bert_mu" % k]) < 1e-5, k
