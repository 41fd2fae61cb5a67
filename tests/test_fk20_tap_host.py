"""The FK20 scalars as an intermediate of the cells' transform (csrc/fr29_ntt.hpp, THE FK20 TAP), without a GPU: the forward network
of the 4096-point transform, run on the host by tests/c/test_fk20_tap.cpp and stopped after its first three radix-4 passes, then the
kernel's own tap, against the definition of the scalars in exact integers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


@pytest.mark.timeout(600)
def test_tapped_values_are_the_fk20_scalars_in_exact_integers(tmp_path):
    """For blob coefficients a and i < 64 the circulant column is v[0] = a[4095 - i], v[1..64] = 0, v[64 + k] = a[64 k - 1 - i] (k = 1..63),
    and scalars[j][i] = scale * NTT_128(v)[j] with omega_128 = omega_8192^64 (k_fk20_scalars; scale = 1/2 in linear-map mode).  All
    128 x 64 of them, from both halves of the extended domain, must be what the tap reads out of the half-finished transform -- each
    (j, i) exactly once.  The vector plants r - 1 at indices 0 and 4095, 0 at 63 and 1 at 64: a wrong c = 63 - i, parity or twiddle
    exponent moves those."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, dump = str(tmp_path / "test_fk20_tap"), str(tmp_path / "tap.txt")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_fk20_tap.cpp"), "-o", exe])
    out = subprocess.run([exe, dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr
    a, got, omega, scale = [], {}, None, None
    for line in open(dump):
        t = line.split()
        if t[0] == "a":
            a.append(int(t[1], 16))
        elif t[0] == "omega":
            omega = int(t[1], 16)
        elif t[0] == "scale":
            scale = int(t[1], 16)
        else:
            key = (int(t[1]), int(t[2]))
            assert key not in got, key
            got[key] = int(t[3], 16)
    assert len(a) == 4096 and len(got) == 8192
    assert omega == pow(7, (R - 1) // 8192, R) and pow(omega, 4096, R) == R - 1 and 2 * scale % R == 1
    assert a[0] == R - 1 and a[4095] == R - 1 and a[63] == 0 and a[64] == 1
    w128 = [pow(omega, 64 * k, R) for k in range(128)]
    for i in range(64):
        v = [0] * 128
        v[0] = a[4095 - i]
        for k in range(1, 64):
            v[64 + k] = a[64 * k - 1 - i]
        nz = [(p, x) for p, x in enumerate(v) if x]
        for j in range(128):
            want = scale * sum(x * w128[p * j % 128] for p, x in nz) % R
            assert got[(j, i)] == want, (j, i)
