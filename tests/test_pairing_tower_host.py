"""csrc/pairing_tower.hpp on the CPU: the tower arithmetic that the host's pairing checks and k_pairing_check share.

A stand-alone program (tests/c/test_pairing_tower.cpp, its own main) built with hipcc's host pass, once plain and once with
AddressSanitizer + UBSan, and run directly: check_lane -- what one lane of the kernel runs -- on pairs whose verdict is known by
construction from the trusted setup's points, against that construction, against product_is_one and, for the Miller value, against the
pieces of the host API.  Nothing is loaded into Python under a sanitizer.  The knob that sends the search's probes to the GPU is parsed
where every knob is (csrc/knobs.hpp)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-eth-kzg_amd", "csrc")
SETUP = os.path.join(ROOT, "rust-eth-kzg_amd", "data", "trusted_setup_4096.bin")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
NAMES = {"valid": 1, "other_scalar": 0, "swapped": 0, "negated": 0, "O_O": 1, "O_X": 0, "X_O": 0}
ROW = re.compile(r"^(\d) (\w+) (\d) want (-?\d) lane (-?\d) host (-?\d) miller (\d)$")


@pytest.fixture(scope="module", params=list(BUILDS))
def rows(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pairing_tower_" + request.param)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp / "test_pairing_tower")
    subprocess.check_call([hipcc, *BUILDS[request.param], "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "test_pairing_tower.cpp"), "-o", exe])
    run = subprocess.run([exe, SETUP], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-3000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert re.match(r"^pairing tower: \d+ cases, 0 mismatches$", lines[-1]), lines[-1]
    got = [ROW.match(l) for l in lines[:-1]]
    assert all(got), [l for l, m in zip(lines, got) if not m][:3]
    return [(int(m[1]), m[2], int(m[3]), int(m[4]), int(m[5]), int(m[6]), int(m[7])) for m in got]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("key", [0, 1])
def test_check_lane_decides_as_the_construction_and_as_the_host(rows, key):
    mine = [r for r in rows if r[0] == key and not r[1].startswith("poison")]
    assert len(mine) == 3 * len(NAMES) * 2  # three positions in the setup, every case normalised and rescaled
    for _, name, rescale, want, lane, host, miller in mine:
        assert want == NAMES[name], name  # the program's list is the list written here
        assert lane == want and host == want, (key, name, rescale, lane, host)
        assert miller == 1, (key, name, rescale)  # bit for bit the host API's Miller value, and the same verdict from it
    assert {(n, r) for _, n, r, *_ in mine} == {(n, r) for n in NAMES for r in (0, 1)}


@pytest.mark.timeout(900)
def test_a_poisoned_slot_is_reported_not_judged(rows):
    mine = [r for r in rows if r[1].startswith("poison")]
    assert len(mine) == 2 * 3 * 2 and {r[1] for r in mine} == {"poison_0", "poison_1"}
    assert all(lane == -1 for _, _, _, _, lane, _, _ in mine)


def test_the_knob_is_parsed_with_the_others(tmp_path):
    src = tmp_path / "knob.cpp"
    src.write_text('#include "knobs.hpp"\n#include <cstdio>\nint main() { printf("%d\\n", kzg::Knobs::from_env().gpu_pairing_min); return 0; }\n')
    exe = str(tmp_path / "knob")
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-I", CSRC, str(src), "-o", exe])
    env = {k: v for k, v in os.environ.items() if k != "ETH_KZG_AMD_GPU_PAIRING_MIN"}
    for value, want in ((None, -1), ("0", 0), ("1", 1), ("300", 300), ("-5", -1), ("junk", 0)):
        e = dict(env)
        if value is not None:
            e["ETH_KZG_AMD_GPU_PAIRING_MIN"] = value
        assert int(subprocess.run([exe], env=e, capture_output=True, text=True, check=True).stdout) == want, value
