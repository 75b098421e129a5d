"""CPU: tools/ot_project_host_check.py at its small shapes -- the OTPROJ-CORE text of csrc/spv_ot_project.h compiled for the CPU behind
the KNN-CORE and OT-CORE texts and held to numpy -- and the marks and names that tool relies on.  No GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_tool_small_shapes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ot_project_host_check.py"), "--small"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all within bounds" in r.stdout and "DIFFERS" not in r.stdout


def test_the_core_text_is_marked_and_names_its_parts():
    text = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_ot_project.h")).read()
    a, b = text.index("// ---- OTPROJ-CORE-BEGIN ----"), text.index("// ---- OTPROJ-CORE-END ----")
    core = text[a:b]
    for name in ("struct OtProj", "otproj_init", "otproj_update", "otproj_merge", "otproj_value", "otproj_ws_rows", "otproj_splits", "otproj_ws_bytes",
                 "otproj_block", "OT_VAL_MAX = 256"):
        assert name in core, name
    for word in ("__global__", "threadIdx", "blockIdx", "__shared__", "atomic"):
        assert word not in core, word
    assert "ot_update(a.st, t)" in core and "ot_merge(a, p)" in core, "(m, sum) goes through spv_ot.h's own update and merge"
    assert "pair_scan<DP>" in text[b:] and "ot_stage_h" in text[b:] and "amdgpu_waves_per_eu(2)" in text[b:]
    assert "atomic" not in text[b:].replace("No floating-point atomics", "")
