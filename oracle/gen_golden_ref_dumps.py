"""Generate the tests/golden fixtures of the differential tests against the reference: the outputs of the reference-side
dump scripts (oracle/ref_*.py) for the exact inputs the tests use, stored so that the tests run without the reference.

    python oracle/gen_golden_ref_dumps.py        (CPU, needs the reference checkout; see oracle/refshim.py)

Writes
  ref_live_cases.npz / ref_live_fullwidth.npz / ref_live_optimus.npz   oracle/ref_live_*.py with the tests' seeds; the
                                  seeded inputs of the first two are dropped (tests/vdtest_util.py draws them again)
  ref_cfg.json.gz                 every model name of the reference's configs/model/*.yaml, resolved by its own bank
  ref_state_dict_layouts.json.gz  state-dict keys and shapes of the full-size reference modules
  ref_schedules.json.gz / ref_schedules_sigmas.npz   the reference's schedule helpers over the tests' grid: one SHA-256
                                  per step count over its bit-exact arrays, the sigmas as values (relative tolerance)
  ref_tokenize.json.gz            the reference's BERT / GPT-2 tokenizers on the tests' random strings
  optimus_vocab_subset.json.gz    the entries of the published BERT vocabulary and GPT-2 vocabulary / merges that the
                                  tokenizer fixtures use, at their published ids / in their published rank order
"""
import gzip
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "versatile-diffusion_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refshim  # noqa: E402
import vdtest_util as U  # noqa: E402  (the inputs the tests feed both sides)


def run(script, args=(), stdin=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", script)] + list(args), input=stdin, capture_output=True,
                       text=True, timeout=3600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def dump_json(name, obj):
    opener = gzip.open if name.endswith(".gz") else open
    with opener(os.path.join(GOLD, name), "wt", encoding="utf-8") as f:
        json.dump(obj, f, sort_keys=True, ensure_ascii=False, separators=(",", ":"))


def _drop_seeded_inputs(d, prefix, inputs):
    """Remove the inputs the tests draw again from their seeds, after checking that they draw exactly these."""
    for name, v in inputs.items():
        assert np.array_equal(d.pop(prefix + name), v.numpy()), prefix + name


def reference_model_names():
    import yaml
    d = os.path.join(refshim.REF_ROOT, "configs", "model")
    names = []
    for fn in sorted(os.listdir(d)):
        if fn.endswith(".yaml"):
            names += list(yaml.safe_load(open(os.path.join(d, fn))))
    return names


def live_npz():
    for script, name, args in (("ref_live_cases.py", "ref_live_cases.npz", ["20260924", "8"]),
                               ("ref_live_fullwidth.py", "ref_live_fullwidth.npz", ["7"]),
                               ("ref_live_optimus.py", "ref_live_optimus.npz", ["31", "6"])):
        tmp = os.path.join(GOLD, name + ".tmp.npz")
        run(script, [tmp] + args)
        d = dict(np.load(tmp))
        os.remove(tmp)
        if name == "ref_live_cases.npz":
            for k in range(int(d["n"])):
                B, _, H, W = d["%d_x" % k].shape
                Hi, Wi = d["%d_img" % k].shape[2:]
                d["%d_dims" % k] = np.array([B, H, W, d["%d_ct" % k].shape[1], d["%d_ci" % k].shape[1], Hi, Wi], dtype=np.int64)
                _drop_seeded_inputs(d, "%d_" % k, U.live_case_inputs(d, k))
        elif name == "ref_live_fullwidth.npz":
            _drop_seeded_inputs(d, "", U.fullwidth_inputs())
        np.savez_compressed(os.path.join(GOLD, name), **d)


def configs_and_layouts():
    out = run("ref_cfg_dump.py", reference_model_names())
    dump_json("ref_cfg.json.gz", json.loads(out[out.index("{"):]))
    out = run("ref_state_dict_dump.py", U.STATE_DICT_MODELS)
    dump_json("ref_state_dict_layouts.json.gz", json.loads(out[out.index('{"'):]))


def schedules():
    out = run("ref_schedules.py", stdin=json.dumps(U.SCHEDULE_GRID))
    ref = json.loads(out[out.index('{"'):])
    sigmas = {}

    def dec(e):
        return np.frombuffer(bytes.fromhex(e["hex"]), dtype=e["dtype"]).reshape(e["shape"])

    ref["betas"] = {k: U.exact_digest([dec(e)]) for k, e in ref["betas"].items()}
    for key, ent in ref["ddim"].items():
        if "error" in ent:
            continue
        exact, errors = [dec(ent["timesteps"])], {}
        for eta in U.SCHEDULE_GRID["etas"]:
            ee = ent["eta%r" % eta]
            if isinstance(ee, dict):
                errors["eta%r" % eta] = ee["error"]
                continue
            sigmas["%s/eta%r" % (key, eta)] = dec(ee[0])
            exact += [dec(ee[1]), dec(ee[2])]
        ref["ddim"][key] = {"sha256": U.exact_digest(exact), "errors": errors}
    dump_json("ref_schedules.json.gz", ref)
    np.savez_compressed(os.path.join(GOLD, "ref_schedules_sigmas.npz"), **sigmas)


class _Recorder(dict):
    """bpe_ranks that remembers every merge the BPE loop applies (it tests `best in bpe_ranks` on the chosen pair only)."""
    def __init__(self, *a):
        super().__init__(*a)
        self.used = set()

    def __contains__(self, k):
        hit = dict.__contains__(self, k)
        if hit:
            self.used.add(k)
        return hit


def tokenizers():
    texts = U.random_tokenizer_texts()
    out = run("ref_tokenize.py", stdin=json.dumps(texts))
    ref = json.loads(out[out.index("{"):])
    dump_json("ref_tokenize.json.gz", {"texts": texts, **ref})
    # vocabulary subsets: every GPT-2 token / merge and every BERT piece the tokenizer fixtures need
    from lib.model_zoo.optimus import optimus_bert_tokenizer, optimus_gpt2_tokenizer
    v = os.path.join(refshim.REF_ROOT, "lib", "model_zoo", "optimus_models", "vocab")
    gpt2 = optimus_gpt2_tokenizer(vocab_file=os.path.join(v, "gpt2-vocab.json"), merges_file=os.path.join(v, "gpt2-merges.txt"))
    gpt2.bpe_ranks = _Recorder(gpt2.bpe_ranks)
    gpt2.add_special_tokens({"pad_token": "<PAD>", "bos_token": "<BOS>", "eos_token": "<EOS>"})
    gcases = json.load(open(os.path.join(GOLD, "optimus_tokenizer.json")))["tokenizer"]["cases"]
    gtexts = texts + [c["text"] for c in gcases] + ["hello", "<BOS> hello <EOS>"]
    ids = set()
    for t in gtexts:
        ids.update(gpt2.encode(t))
    inv = {i: t for t, i in gpt2.encoder.items()}
    ranks = sorted((r, k) for k, r in dict.items(gpt2.bpe_ranks) if k in gpt2.bpe_ranks.used)
    sub = {"gpt2": {"len": len(gpt2.encoder), "unk": [gpt2.unk_token, gpt2.encoder[gpt2.unk_token]],
                    "tokens": {inv[i]: i for i in sorted(ids) if i in inv}, "merges": [" ".join(k) for _, k in ranks]}}
    bert_meta = json.load(open(os.path.join(GOLD, "optimus_bert_tokenizer.json")))["tokenizer"]
    pieces = set()
    for lower, cases in ((False, texts + [c["text"] for c in bert_meta["cases"]]), (True, [c["text"] for c in bert_meta["cases_lower"]])):
        tok = optimus_bert_tokenizer(vocab_file=os.path.join(v, "bert-base-cased-vocab.txt"), do_lower_case=lower, max_len=512)
        for t in cases:
            pieces.update(tok.tokenize(t))
    pieces.update(tok.all_special_tokens)
    sub["bert"] = {"len": len(tok.vocab), "pieces": {p: tok.vocab[p] for p in sorted(pieces)}}
    dump_json("optimus_vocab_subset.json.gz", sub)


if __name__ == "__main__":
    assert refshim.reference_available(), "needs the reference checkout"
    which = sys.argv[1:] or ["live", "cfg", "schedules", "tokenizers"]
    for w in which:
        {"live": live_npz, "cfg": configs_and_layouts, "schedules": schedules, "tokenizers": tokenizers}[w]()
        print("wrote", w)
