"""CPU: tools/tsne_host_check.py at its small shapes -- the TSNE-CORE text of csrc/spv_tsne.h compiled for the CPU behind the KNN-CORE text
and held to numpy -- and the marks and names that tool relies on.  No GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_tool_small_shapes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tsne_host_check.py"), "--small"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all within bounds" in r.stdout and "DIFFERS" not in r.stdout


def test_the_core_text_is_marked_and_names_its_parts():
    text = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_tsne.h")).read()
    a, b = text.index("// ---- TSNE-CORE-BEGIN ----"), text.index("// ---- TSNE-CORE-END ----")
    core = text[a:b]
    for name in ("tsne_w", "struct TsneSums", "tsne_add", "tsne_merge", "tsne_splits", "tsne_ws_bytes", "tsne_calibrate", "tsne_attract", "tsne_grad",
                 "tsne_step", "tsne_zsum_lane", "TSNE_DMAX = 4"):
        assert name in core, name
    for word in ("__global__", "threadIdx", "blockIdx", "__shared__", "atomic"):
        assert word not in core, word
    assert "knn_d2(" in core, "the pair's distance is spv_knn's chain"
    assert "pair_scan<TSNE_DMAX>" in text[b:] and "tsne_add(s, q, cv, d2)" in text[b:]
    assert "atomic" not in text[b:]
