"""LoRA adapters (Hu et al. 2021; not in the reference): merged into the weights on the device, between calls.

    tensors = lora.load_file("style.pt")
    lora.attach(net, "style", tensors)              # parse + validate against net; nothing is written yet
    lora.set_adapters(net, {"style": 0.75})         # exactly these adapters at these strengths; {} = none
    lora.detach(net, "style")

An adapter adds scale * (alpha / r) * up @ down to the weight of chosen nn.Linear / nn.Conv2d (groups == 1) modules anywhere in the
model.  set_adapters recomputes every layer whose active terms changed FROM A KEPT BASE with one ops.lora_merge launch (contract
with written-out roundings: include/vd_hip.h, vd_lora_merge), so the parameter bits depend on the active set alone, never on the
history of switches, and the empty set gives the base bits back.  The parameter is written with param.copy_(), which advances its
version: the next forward rebuilds the kernel-layout packs of the touched layers only (hip_layers.PackCache), and the next sample()
captures a new step graph (ddim._static_key).  Switching is a between-calls operation: it must not run while another thread's
forward does.  State lives on the model object (net._vd_lora); the module is function-based.
"""
import collections
import math

import numpy as np
import torch
import torch.nn as nn

from vd_hip import loader, ops

MAX_TERMS, MAX_RANK = ops.LORA_MAX_TERMS, ops.LORA_MAX_RANK
FLAT_PREFIX = "lora_vd_"
# key suffix -> role: native (kohya-style) and PEFT names of the pair
_SUFFIXES = ((".lora_down.weight", "down"), (".lora_up.weight", "up"), (".lora_A.weight", "down"), (".lora_B.weight", "up"),
             (".alpha", "alpha"))


class _Layer(object):
    """What is kept per touched module: the base snapshot (None until a term first touches the layer), the terms last written
    ((adapter name, fp32 scale) in attach order) and the parameter's (data_ptr, _version) behind that write."""

    def __init__(self, module):
        self.module, self.base, self.applied, self.stamp = module, None, (), None


class _State(object):
    def __init__(self):
        self.adapters = collections.OrderedDict()   # name -> {path: (up [N, r], down [r, K], alpha / r as a float)}
        self.layers = {}                            # path -> _Layer
        self.active = collections.OrderedDict()     # name -> scale as given


def _state(net, create=False):
    st = net.__dict__.get("_vd_lora")
    if st is None and create:
        st = net.__dict__["_vd_lora"] = _State()
    return st


def _stamp(w):
    return (w.data_ptr(), w._version)


def load_file(path):
    """A dict of tensors from an adapter file: torch.save files, and .safetensors where the safetensors package is installed."""
    path = str(path)
    if path.lower().endswith(".safetensors"):
        try:
            from safetensors.torch import load_file as st_load
        except ImportError:
            raise RuntimeError("lora.load_file: %s needs the safetensors package, which is not installed; "
                               "convert the file to a torch.save file or install safetensors" % path)
        return dict(st_load(path, device="cpu"))
    obj = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(obj, dict) or not all(isinstance(k, str) for k in obj):
        raise ValueError("lora.load_file: %s does not hold a dict of named tensors" % path)
    return dict(obj)


def targets(net):
    """{module path: module} of everything an adapter can name: nn.Linear and nn.Conv2d with groups == 1."""
    return {p: m for p, m in net.named_modules()
            if p and (isinstance(m, nn.Linear) or (isinstance(m, nn.Conv2d) and m.groups == 1))}


def flat_key(path):
    return FLAT_PREFIX + path.replace(".", "_")


def _split_key(key):
    for suffix, role in _SUFFIXES:
        if key.endswith(suffix) and len(key) > len(suffix):
            return key[:-len(suffix)], role
    raise ValueError("lora.attach: key %r matches no form (<path>.lora_down.weight / .lora_up.weight / .alpha, "
                     "<path>.lora_A.weight / .lora_B.weight, %s<flattened path>.*)" % (key, FLAT_PREFIX))


def parse(net, tensors, alpha=None, strict=True):
    """The plan of an adapter against `net`, on the host: {path: (up [N, r] fp32, down [r, K] fp32, alpha / r)} in the order of
    net.named_modules().  Raises ValueError (see attach) and touches no device."""
    tg = targets(net)
    flat = {}
    for p in tg:
        flat.setdefault(flat_key(p), []).append(p)
    raw = {}
    for key, val in tensors.items():
        prefix, role = _split_key(str(key))
        if prefix.startswith(FLAT_PREFIX):
            paths = flat.get(prefix, [])
            if len(paths) > 1:
                raise ValueError("lora.attach: %r is ambiguous: it flattens %s" % (key, " and ".join(paths)))
            path = paths[0] if paths else None
        else:
            path = prefix if prefix in tg else None
        if path is None:
            if strict:
                raise ValueError("lora.attach: %r names no nn.Linear / nn.Conv2d (groups == 1) of the model" % (key,))
            continue
        slot = raw.setdefault(path, {})
        if role in slot:
            raise ValueError("lora.attach: %r repeats the %s of %s" % (key, role, path))
        slot[role] = val
    plan = collections.OrderedDict()
    for path in tg:
        if path not in raw:
            continue
        slot, mod = raw[path], tg[path]
        if "up" not in slot or "down" not in slot:
            raise ValueError("lora.attach: %s has %s without its %s" % (path, " and ".join(sorted(slot)),
                                                                        "down" if "down" not in slot else "up"))
        up, down = slot["up"], slot["down"]
        for t, what in ((up, "up"), (down, "down")):
            if not isinstance(t, torch.Tensor) or not t.is_floating_point():
                raise ValueError("lora.attach: the %s of %s is not a floating-point tensor" % (what, path))
        if isinstance(mod, nn.Conv2d):
            kh, kw = mod.kernel_size
            want_down, want_up = (mod.in_channels, kh, kw), (mod.out_channels,)
            ok = (down.dim() == 4 and up.dim() == 4 and tuple(down.shape[1:]) == want_down
                  and tuple(up.shape[2:]) == (1, 1) and up.shape[0] == mod.out_channels)
            shapes = "down [r, %d, %d, %d] and up [%d, r, 1, 1]" % (want_down + want_up)
        else:
            ok = down.dim() == 2 and up.dim() == 2 and down.shape[1] == mod.in_features and up.shape[0] == mod.out_features
            shapes = "down [r, %d] and up [%d, r]" % (mod.in_features, mod.out_features)
        if not ok:
            raise ValueError("lora.attach: %s takes %s, got down %s and up %s" % (path, shapes, tuple(down.shape), tuple(up.shape)))
        r = int(down.shape[0])
        if int(up.shape[1]) != r:
            raise ValueError("lora.attach: rank mismatch at %s: down has %d rows, up %d columns" % (path, r, int(up.shape[1])))
        if not 1 <= r <= MAX_RANK:
            raise ValueError("lora.attach: rank %d at %s outside 1..%d" % (r, path, MAX_RANK))
        a = slot.get("alpha", alpha)
        if isinstance(a, torch.Tensor):
            if a.numel() != 1:
                raise ValueError("lora.attach: the alpha of %s is not a scalar" % path)
            a = a.double().item()
        a = float(r) if a is None else float(a)
        if not math.isfinite(a):
            raise ValueError("lora.attach: the alpha of %s is not finite" % path)
        up32 = up.detach().to(torch.float32).reshape(up.shape[0], r).contiguous()        # fp16 / bf16 widen exactly
        down32 = down.detach().to(torch.float32).reshape(r, -1).contiguous()
        if not (bool(torch.isfinite(up32).all()) and bool(torch.isfinite(down32).all())):
            raise ValueError("lora.attach: non-finite values at %s" % path)
        plan[path] = (up32, down32, a / r)
    return plan


def attach(net, name, tensors, alpha=None, strict=True):
    """Parse and validate an adapter against `net` and keep it under `name`; it is not activated.  Keys: <path>.lora_down.weight /
    <path>.lora_up.weight / optional scalar <path>.alpha (native), <path>.lora_A.weight / <path>.lora_B.weight (PEFT), or
    lora_vd_<path with '.' -> '_'>.* (flattened), <path> a module path of net.named_modules().  Linear: down [r, in], up [out, r];
    Conv2d: down [r, Cin, kh, kw], up [Cout, r, 1, 1].  The factor is alpha / r with alpha from the file, else the argument, else r.
    The tensors are kept as contiguous fp32 on the parameter's device.  ValueError, before anything touches the device, for a
    duplicate name, a key of no form, (strict) a path that is no such module, an ambiguous flattening, half a pair, a rank
    mismatch, a shape that does not fit the layer, r outside 1..256, non-finite values or alpha.  Returns the paths it names."""
    st = _state(net)
    if st is not None and name in st.adapters:
        raise ValueError("lora.attach: an adapter named %r is attached already" % (name,))
    plan = parse(net, tensors, alpha, strict)
    tg = targets(net)
    st = _state(net, create=True)
    entry = collections.OrderedDict()
    for path, (up, down, factor) in plan.items():
        dev = tg[path].weight.device
        entry[path] = (up.to(dev), down.to(dev), factor)
        if path not in st.layers:
            st.layers[path] = _Layer(tg[path])
    st.adapters[name] = entry
    return list(entry)


def term_scale(strength, factor):
    """The fp32 scale of a term: strength * (alpha / r) in float64, rounded once."""
    return float(np.float32(float(strength) * float(factor)))


def set_adapters(net, scales):
    """Make exactly the adapters of `scales` ({name: strength}) active; {} = none.  A layer whose terms ((name, fp32 scale) in attach
    order) did not change is not written.  ValueError for an unknown name, a non-finite strength or more than 8 active terms on one
    layer; RuntimeError when the weights of a layer with active terms were edited by someone else since the last call (call
    reset(net) first), when the parameters are not on a GPU or when the kernel library is missing.  Nothing is written when it
    raises."""
    st = _state(net, create=True)
    scales = dict(scales)
    for name, s in scales.items():
        if name not in st.adapters:
            raise ValueError("lora.set_adapters: no adapter named %r is attached" % (name,))
        if not isinstance(s, (int, float)) or not math.isfinite(float(s)):
            raise ValueError("lora.set_adapters: the scale of %r is not a finite number" % (name,))
    todo = []
    for path, lay in st.layers.items():
        want = tuple((name, term_scale(scales[name], entry[path][2])) for name, entry in st.adapters.items()
                     if name in scales and path in entry)
        if len(want) > MAX_TERMS:
            raise ValueError("lora.set_adapters: %d active terms on %s, at most %d" % (len(want), path, MAX_TERMS))
        w = lay.module.weight
        edited = lay.stamp is not None and lay.stamp != _stamp(w)
        if edited and lay.applied:
            raise RuntimeError("lora.set_adapters: the weight of %s was changed (load_state_dict, .half(), .to(), an in-place edit) "
                               "while adapters were merged into it; call lora.reset(net) and attach again" % path)
        if edited:                      # nothing of ours in it: what is there now is the new base
            lay.base, lay.stamp = None, None
        if want != lay.applied:
            todo.append((path, lay, want))
    if any(want for _, _, want in todo):
        loader.lib()                    # raises VdHipError (a RuntimeError) when the library is not built
        for path, lay, want in todo:
            if want and not lay.module.weight.is_cuda:
                raise ops.VdHipError("lora.set_adapters: the weight of %s must live on the GPU (no CPU fallback in the product path)" % path)
    with torch.no_grad():
        for path, lay, want in todo:
            w = lay.module.weight
            if not want:
                w.copy_(lay.base)
            else:
                if lay.base is None:
                    lay.base = w.detach().clone(memory_format=torch.contiguous_format)
                terms = []
                for name, s32 in want:
                    up, down, factor = st.adapters[name][path]
                    if up.device != w.device:       # the model moved since attach
                        up, down = up.to(w.device), down.to(w.device)
                        st.adapters[name][path] = (up, down, factor)
                    terms.append((up, down, s32))
                merged = ops.lora_merge(lay.base.view(lay.base.shape[0], -1), terms)
                w.copy_(merged.view(w.shape))       # advances w._version: packs and kept graphs notice
            lay.applied, lay.stamp = want, _stamp(w)
    st.active = collections.OrderedDict((name, float(scales[name])) for name in st.adapters if name in scales)


def detach(net, name):
    """Remove an adapter; an active one is switched off first (as set_adapters without it).  The base of a layer no other adapter
    names is let go."""
    st = _state(net)
    if st is None or name not in st.adapters:
        raise ValueError("lora.detach: no adapter named %r is attached" % (name,))
    if name in st.active:
        set_adapters(net, {n: s for n, s in st.active.items() if n != name})
    del st.adapters[name]
    named = set(p for entry in st.adapters.values() for p in entry)
    for path in [p for p in st.layers if p not in named]:
        del st.layers[path]


def active(net):
    """{name: scale} of the active adapters, in attach order."""
    st = _state(net)
    return {} if st is None else dict(st.active)


def attached(net):
    """The names of the attached adapters, in attach order."""
    st = _state(net)
    return [] if st is None else list(st.adapters)


def reset(net):
    """Forget every adapter and base WITHOUT writing a parameter: whatever the weights hold now is what the model is."""
    net.__dict__.pop("_vd_lora", None)
