"""Resource guard for the ame_smooth kernels (no GPU needed): compiles
ame_smooth.hip for gfx950 and reads the compiler's resource report.

The solve kernel is not templated on r (d is a runtime value), so one instance
serves r = 16 and r = 32 alike; its LDS is the static part the report shows
plus the dynamic part the library sizes per r (ame_smooth_lds_bytes).  A
scratch spill in its matrix loops would turn every LDS-resident product into
memory traffic, so none is allowed in any of the four kernels.  (SGPRs the
compiler parks in VGPR lanes are not scratch: the solve kernel has 28 of them,
its 17 arguments and the uniform loop state of both passes.)
"""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(__file__), "..", "python-temporal-ame-svi_amd", "ame_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
LDS_MAX = 163840


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_smooth_kernels_have_no_spills_and_fit_lds(tmp_path):
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
    for part in ("ame_smooth_gram_kernel", "ame_smooth_h_kernel", "ame_smooth_solve_kernel",
                 "ame_smooth_lag_kernel"):
        names = [k for k in report if part in k]
        assert names, f"no resource report for {part}: {list(report)}"
        for name in names:
            rep = report[name]
            assert rep.get("VGPRs Spill") == 0, (name, rep)
            assert rep.get("ScratchSize", 0) == 0, (name, rep)
            assert rep.get("LDS Size", 0) <= 65536, (name, rep)      # static LDS
    solve = report[next(k for k in report if "ame_smooth_solve_kernel" in k)]
    from ame_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from ame_amd.build import build
        build(verbose=False)
    for r_ in (16, 32):
        total = solve.get("LDS Size", 0) + int(L.lib().ame_smooth_lds_bytes(r_))
        assert total <= LDS_MAX, (r_, total)
    assert solve.get("Occupancy", 0) >= 4, solve   # r = 16: four 39 KB workgroups share a CU
