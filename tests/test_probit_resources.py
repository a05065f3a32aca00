"""Resource guard for the binary-network kernels (no GPU needed): compiles
ame_binary.hip, and ame_predict.hip at the widest latent dim, for gfx950 and
reads the compiler's resource report.  The fill kernel has no scratch at all;
the scoring mode has none beyond what the shared tile kernel already has.

ame_probit_fill_kernel runs an fp64 recursion with six erfcx per pair next to
two MFMA accumulators; a scratch spill there would put memory traffic into the
part that sets its time.  Its LDS (operand panels, one 64 x 16 strip of the tile
in both orientations, the words) must leave room for two workgroups per CU and
stay within the 64 KB a workgroup may declare statically.
"""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(__file__), "..", "python-temporal-ame-svi_amd", "ame_amd", "csrc")
INC = os.path.join(os.path.dirname(__file__), "..", "include")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


def _report(src, out, extra=()):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", f"-I{CSRC}", f"-I{INC}",
           "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", *extra, "-c",
           os.path.join(CSRC, src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    report, current = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            current = m.group(1)
            report[current] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and current is not None:
            report[current][m.group(1).strip()] = int(m.group(2))
    return report


def _check(report, part, scratch=0):
    names = [k for k in report if part in k]
    assert names, f"no resource report for {part}: {list(report)}"
    for name in names:
        rep = report[name]
        assert rep.get("VGPRs Spill") == 0, (name, rep)
        assert rep.get("ScratchSize", 0) <= scratch, (name, rep)
        assert rep.get("LDS Size", 0) <= 65536, (name, rep)
    return [report[k] for k in names]


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_probit_fill_kernel_has_no_scratch_and_fits_lds(tmp_path):
    rep, = _check(_report("ame_binary.hip", tmp_path / "pb.o"), "ame_probit_fill_kernel")
    assert rep.get("Occupancy", 0) >= 2, rep   # two 57 KB workgroups share a CU


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_probit_score_kernel_has_no_scratch_and_fits_lds(tmp_path):
    """MODE 3 adds an epilogue to the tile kernel every mode shares.  That body
    keeps its four staging pointers (gi[2], gj[2]) in 32 bytes of scratch in every
    mode; the Bernoulli epilogue must add none to it and spill no VGPR."""
    report = _report("ame_predict.hip", tmp_path / "pr.o", ("-DAME_ONLY_R=32",))
    base, = _check(report, "ame_predict_pairs_kernelILi32ELi0EE", scratch=32)   # <32, 0>: Gaussian scoring
    rep, = _check(report, "ame_predict_pairs_kernelILi32ELi3EE", scratch=base.get("ScratchSize", 0))
    assert rep.get("Occupancy", 0) >= base.get("Occupancy", 0), (rep, base)
