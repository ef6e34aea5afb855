"""Host-side surface of the shared head of the first context block under classifier-free guidance (no GPU needed): the
descriptor keeps its layout, the new entry point is declared on both sides of the C ABI, the switch is documented."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_ff_chain_descriptor_keeps_its_layout():
    """period_rows takes the slot of the former `reserved` word: same size, same offsets, zero = off (what every caller that
    cleared the descriptor has been passing)."""
    from vd_hip.loader import VdFfChain
    assert ctypes.sizeof(VdFfChain) == 152
    assert VdFfChain.period_rows.offset == 148 and VdFfChain.period_rows.size == 4
    assert VdFfChain.alpha.offset == 144 and VdFfChain.M.offset == 128 and VdFfChain.stat_img_rows.offset == 120
    assert VdFfChain().period_rows == 0
    hdr = _read("include", "vd_hip.h")
    body = hdr[hdr.index("typedef struct VdFfChain {"):hdr.index("} VdFfChain;")]
    fields = re.findall(r"(\w+)\s*(?:,\s*(\w+)\s*)?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    names = [n for pair in fields for n in pair if n]
    assert names == [n for n, _ in VdFfChain._fields_]
    assert re.search(r"#define VD_HIP_ABI_VERSION 8\b", hdr)


def test_xattn_rep_entry_is_declared_like_the_plain_one_plus_the_sample_count():
    from vd_hip.loader import PROTOTYPES
    plain, rep = PROTOTYPES["vd_xattn_f16"], PROTOTYPES["vd_xattn_rep_f16"]
    assert rep[0] is plain[0] and len(rep[1]) == len(plain[1]) + 1
    assert rep[1][:9] == plain[1][:9] and rep[1][9] is ctypes.c_int and rep[1][10:] == plain[1][9:]
    hdr = _read("include", "vd_hip.h")
    m = re.search(r"int vd_xattn_rep_f16\(([^;]*)\);", hdr)
    assert m and re.search(r"int B,\s*int x_samples,\s*int H", m.group(1))
    assert "vd_xattn_rep_f16" in _read("INTEGRATION.md")


def test_switch_is_on_by_default_and_documented():
    from lib.model_zoo import vd
    assert vd.CFG_HEAD_SHARE is (os.environ.get("VD_CFG_HEAD_SHARE", "1") != "0")
    assert "VD_CFG_HEAD_SHARE" in _read("tools", "README.md")
