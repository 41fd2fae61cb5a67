"""The G1 endomorphism in the compiled linear map (csrc/g1_linmap.hpp: Toom-Cook points on the sixth roots of unity, rotations
as operand modifiers that k_g1slp.hip applies with curve30.hpp's apply_phi).  Host only: tests/c/test_linmap_phi.cpp built
with hipcc's host pass, no GPU involved."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")


@pytest.mark.timeout(600)
def test_phi_plans_match_definition_and_phi_is_lambda(tmp_path):
    """phi(X : Y : Z) = (beta X : Y : Z) on the signed points equals [lambda] P of the saturated group law (also phi^2, additions
    with a rotated operand, P + phi(P) = -phi^2(P)); every strategy's plan and each schedule form equal the map's definition over
    Fr; the tuned plan's operation counts are printed, and the plan on mu_6 is the one with fewer constant multiplications."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "test_linmap_phi")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_linmap_phi.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout
    assert re.search(r"phi on JacS: [1-9]\d* checks", out.stdout)
    counts = {int(m.group(1)): (int(m.group(2)), float(m.group(3))) for m in re.finditer(
        r"strategy tuned=1 phi=(\d) splits 0 0 0 0: (\d+) mulc.*cost ([\d.]+) M", out.stdout)}
    assert set(counts) == {0, 1}
    assert counts[1][0] < counts[0][0] and counts[1][1] < counts[0][1]
