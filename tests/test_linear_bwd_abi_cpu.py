"""CPU: the pending-reduce record of spv_linear_bwd has the size and field offsets of its ctypes mirror (plain gcc against
include/spvipes_hip.h, no GPU), and the Python constants that size its workspace are the kernel's."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pending_record_layout_matches_the_header(tmp_path):
    from spvipes_amd import _abi

    fields = {"spv_linear_pending": ("p", "nprob", "wpart", "prob_stride"), "spv_linear_pending_prob": ("dW", "db", "N", "K")}
    mirrors = {"spv_linear_pending": _abi.SpvLinearPending, "spv_linear_pending_prob": _abi.SpvLinearPendingProb}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "spvipes_hip.h")}"', "int main(void) {"]
    for n, fs in fields.items():
        lines.append(f'  printf("{n} %zu\\n", sizeof({n}));')
        lines += [f'  printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for f in fs]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "pending.c", tmp_path / "pending"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, fs in fields.items():
        assert int(got[n]) == ctypes.sizeof(mirrors[n]), n
        for f in fs:
            assert int(got[f"{n}.{f}"]) == getattr(mirrors[n], f).offset, (n, f)


def test_workspace_constants_are_the_kernels():
    from spvipes_amd import _abi

    src = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_small.h")).read()
    assert int(re.search(r"constexpr int WG_SLICES = (\d+);", src).group(1)) == _abi.WG_SLICES
    assert int(re.search(r"constexpr int WG_DIRECT_MAX_B = (\d+);", src).group(1)) == _abi.WG_DIRECT_MAX_B
