"""Child process of tests/test_exact_attention_gpu.py::test_attn_fwd_kernel_8_waves_in_a_child_process: with VD_ATTN_PIPE=0 in
the environment (the library reads it once per process) the attn_pipe_kernel shapes run on attn_fwd_kernel<40, 8>.  Prints one
line per case and the report of every mismatch; exit status 1 on a mismatch."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "versatile-diffusion_amd")):      # the way the suite's modules are found
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    assert os.environ.get("VD_ATTN_PIPE") == "0", "VD_ATTN_PIPE=0 must be set before the library is loaded"
    import torch
    import attn_cases as A
    from vd_hip import ops
    from vdtest_util import attn_mismatch
    dev = torch.device("cuda:0")
    failed = 0
    for name in A.names("pipe"):
        t = A.build(name)
        c = t.case
        out = ops.attention(t.q.to(dev), t.k.to(dev), t.v.to(dev), c["H"]).cpu().view(c["B"], c["Nq"], c["H"], c["D"])
        msg = attn_mismatch(out, t.ref, name + " (VD_ATTN_PIPE=0)", win_key=t.pi, qblock=256, wave_rows=32)
        print("%s: %s" % (name, "ok" if msg is None else "MISMATCH\n" + msg))
        failed += msg is not None
    if not failed:
        print("all cases pass")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
