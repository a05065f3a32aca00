"""Resource guard for ame_smooth_hgram_kernel (no GPU needed): compiles
ame_smooth.hip for gfx950 and reads the compiler's resource report.

The kernel keeps the lower-triangle tiles of the hidden partners' Gram matrix
in registers (1, 3, 6 or 10 tiles of four fp64 values per lane): a spill would
turn every MFMA step into scratch traffic, so none is allowed in any of the
four instances, and the kernel uses no LDS.
"""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(__file__), "..", "python-temporal-ame-svi_amd", "ame_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_hgram_instances_have_no_spills_and_no_scratch(tmp_path):
    src = os.path.join(CSRC, "ame_smooth.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", f"-I{CSRC}",
           "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src,
           "-o", str(tmp_path / "sm.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    report = {}
    current = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            current = m.group(1)
            report[current] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and current is not None:
            report[current][m.group(1).strip()] = int(m.group(2))
    names = [k for k in report if "ame_smooth_hgram_kernel" in k]
    assert len(names) == 4, names     # tile counts 1 .. 4
    for name in names:
        rep = report[name]
        print(name, rep)
        assert rep.get("VGPRs Spill") == 0, (name, rep)
        assert rep.get("SGPRs Spill", 0) == 0, (name, rep)
        assert rep.get("ScratchSize", 0) == 0, (name, rep)
        assert rep.get("LDS Size", 0) == 0, (name, rep)
        assert rep.get("Occupancy", 0) >= 4, (name, rep)   # 10 tiles = 80 accumulator registers at most
