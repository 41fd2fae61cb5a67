"""The Reed-Solomon decoder of recovery on its own (Engine::rs_decode through eth_kzg_amd_test_rs_decode: k_rec_vanishing_poly,
k_rec_vanishing, k_cells_to_fr, k_rec_dit_half / _last, k_rec_dif_half), stage by stage against exact integers (tests/rs_reference.py).

A whole recovery cannot see a wrong vanishing polynomial: the decoder only needs Z to vanish on the missing cells and to be non-zero on
the coset, so a wrong scalar, an extra root on a present cell or a wrong zp[64] still decodes whenever more than 64 cells are present.
Here deg, all 65 coefficients of Z', its 128 values and 128 inverse coset values are compared byte for byte at every erasure count
0 .. 64, and the coefficients with the polynomial the cells were made from.  No tolerances: everything is integer work.

Run on the MI355X box:  python -m pytest tests/test_gpu_rs_decode.py -m gpu -x -q
"""
import ctypes as C
import importlib
import random

import pytest

import rs_reference as F
from oracle_lib import OracleError

pytestmark = pytest.mark.gpu
kzg = importlib.import_module("rust-eth-kzg_amd")

R = F.R
CELL = 2048
FF_CELL = b"\xff" * CELL


@pytest.fixture(scope="module")
def ctx():
    import torch
    torch.cuda.init()  # torch initialises its HIP state before the engine creates its streams
    c = kzg.DASContext(use_precomp=False)
    if not hasattr(c._lib, "eth_kzg_amd_test_rs_decode"):
        pytest.fail("the test hooks library (libc_eth_kzg_hooks.so) is not the library loaded")
    yield c
    c.close()


# ---- the hook ----------------------------------------------------------------------------------------------------------------------------
class Decoded:
    def __init__(self, rc, n, status, deg, zp, zeval, zcinv, coeffs):
        self.rc, self.n = rc, n
        self.status, self.deg = list(status)[:n], list(deg)[:n]
        self.raw = (zp.raw, zeval.raw, zcinv.raw, coeffs.raw)

    def _ints(self, which, r, count):
        raw = self.raw[which]
        return [int.from_bytes(raw[32 * (r * count + k):32 * (r * count + k + 1)], "big") for k in range(count)]

    def zp(self, r):
        return self._ints(0, r, 65)

    def zeval(self, r):
        return self._ints(1, r, 128)

    def zcinv(self, r):
        return self._ints(2, r, 128)

    def coeffs(self, r):
        return self._ints(3, r, 4096)

    def coeff_bytes(self, r):
        return self.raw[3][r * 4096 * 32:(r + 1) * 4096 * 32]


def rs_decode(handle, blobs, flat=False, junk=FF_CELL, counts=None):
    """blobs = [(present cell indices, {cell index: 2048 bytes})]: the hook's list form, or its flat form with every absent cell (or the
    cells `junk` maps, when it is a dict per blob) holding junk.  counts overrides n_cells (the refused-count cases)."""
    lib = kzg.load_library()
    n = len(blobs)
    keep = []
    nc = (C.c_uint64 * n)(*[len(idx) if counts is None else counts[b] for b, (idx, _) in enumerate(blobs)])
    ipp, cpp = (C.c_void_p * n)(), (C.c_void_p * n)()
    for b, (idx, cells) in enumerate(blobs):
        ia = (C.c_uint64 * max(1, len(idx), nc[b]))(*idx)
        if flat:
            fill = junk[b] if isinstance(junk, list) else {}
            default = junk if isinstance(junk, bytes) else FF_CELL
            have = set(idx)
            buf = C.create_string_buffer(b"".join(cells[c] if c in have else fill.get(c, default) for c in range(128)), 128 * CELL)
            ca = (C.c_void_p * 1)(C.addressof(buf))
            keep.append(buf)
        else:
            bufs = [C.create_string_buffer(cells[c], CELL) for c in idx]
            ca = (C.c_void_p * max(1, len(bufs), nc[b]))(*[C.addressof(x) for x in bufs] + [C.addressof(bufs[0])] * max(0, nc[b] - len(bufs)))
            keep.append(bufs)
        keep += [ia, ca]
        ipp[b], cpp[b] = C.addressof(ia), C.addressof(ca)
    status, deg = (C.c_int32 * n)(*[-1] * n), (C.c_int32 * n)(*[-1] * n)
    zp, zeval, zcinv = C.create_string_buffer(n * 65 * 32), C.create_string_buffer(n * 128 * 32), C.create_string_buffer(n * 128 * 32)
    coeffs = C.create_string_buffer(n * 4096 * 32)
    rc = lib.eth_kzg_amd_test_rs_decode(handle, n, nc, ipp, cpp, int(flat), status, deg, zp, zeval, zcinv, coeffs)
    return Decoded(rc, n, status, deg, zp, zeval, zcinv, coeffs)


# ---- polynomials and placements ------------------------------------------------------------------------------------------------------------
def _random_poly(seed, n=4096):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


POLYS = {  # at most six across the 130 blobs of the erasure-count calls
    "zero": [0] * 4096,
    "seven": [7] + [0] * 4095,
    "x^4095": [0] * 4095 + [1],
    "all r-1": [R - 1] * 4096,
    "random a": _random_poly("rs-decode a"),
    "random b": _random_poly("rs-decode b"),
}
_cells = {}  # polynomial name -> its 128 cells: computed once, shared, never changed


def cells_of(name):
    if name not in _cells:
        _cells[name] = F.extend(POLYS[name])
    return _cells[name]


def _run(start, d):
    return list(range(start, start + d))


def _centred(at, d):
    """d contiguous domain indices around the boundary at - 1 / at (both sides of it from d = 2)"""
    return _run(at - (d + 1) // 2, d)


def placement(call, d):
    """(kind, missing domain indices) of the blob with d missing cells in erasure-count call 0 or 1"""
    if d == 0:
        return "none", []
    kind = d % 3
    if call == 0:
        if kind == 1:
            return "from 0", _run(0, d)
        if kind == 2:
            return "straddles 31/32", _centred(32, d)
        return "random", sorted(random.Random("rs-decode call 0 / %d" % d).sample(range(128), d))
    if kind == 1:
        return "up to 127", _run(128 - d, d)
    if kind == 2:
        return ("straddles 63/64", _centred(64, d)) if d % 2 == 0 else ("straddles 95/96", _centred(96, d))
    return "random", sorted(random.Random("rs-decode call 1 / %d" % d).sample(range(128), d))


def erasure_call(call):
    """[(polynomial name, missing domain indices, present cells)] for d = 0 .. 64"""
    names = list(POLYS)
    out = []
    for d in range(65):
        _, missing = placement(call, d)
        gone = set(F.cells_of_domain_indices(missing))
        out.append((names[(d + 3 * call) % 6], missing, [c for c in range(128) if c not in gone]))
    return out


def test_the_placements_are_the_ones_asked_for():
    seen = {}
    for call in (0, 1):
        for d in range(65):
            kind, missing = placement(call, d)
            assert len(missing) == d == len(set(missing)) and all(0 <= i < 128 for i in missing), (call, d)
            seen.setdefault(kind, []).append(missing)
    assert placement(0, 1)[1] == [0] and placement(1, 1)[1] == [127]  # domain index 0 alone, 127 alone
    assert _run(0, 64) in seen["from 0"] and _run(64, 64) in seen["up to 127"]
    for kind, lo in (("straddles 31/32", 31), ("straddles 63/64", 63), ("straddles 95/96", 95)):
        assert seen[kind] and all(lo in m and lo + 1 in m and m == _run(m[0], len(m)) for m in seen[kind]), kind
    assert max(len(m) for m in seen["straddles 31/32"]) == 62 and [31, 32] in seen["straddles 31/32"]
    assert len(seen["random"]) >= 40 and placement(0, 33)[0] == "random" and placement(0, 32)[0] == "straddles 31/32"
    assert placement(0, 31)[0] == "from 0" and placement(0, 63)[0] == "random" and placement(0, 64)[0] == "from 0"
    for call in (0, 1):
        assert {p for p, _, _ in erasure_call(call)} == set(POLYS)


_erasures = {}  # call -> (blobs, Decoded of the list form): decoded once, shared with the flat-source test


def _decode_erasures(ctx, call):
    if call not in _erasures:
        plan = erasure_call(call)
        blobs = [(present, cells_of(name)) for name, _, present in plan]
        _erasures[call] = (blobs, rs_decode(ctx.handle, blobs))
    return _erasures[call]


@pytest.mark.parametrize("call", [0, 1])
def test_every_erasure_count(ctx, call):
    plan = erasure_call(call)
    _, got = _decode_erasures(ctx, call)
    assert got.rc == 0
    bad = []
    for d, (name, missing, present) in enumerate(plan):
        assert len(present) == 128 - d
        z = F.vanishing(missing)
        kind = placement(call, d)[0]
        if got.deg[d] != d:
            bad.append((d, kind, "deg", got.deg[d]))
        zp = got.zp(d)
        if zp != z:
            bad.append((d, kind, "zp", [k for k in range(65) if zp[k] != z[k]]))
        want = [F.vanishing_at_cell(z, c) for c in range(128)]
        ze = got.zeval(d)
        if ze != want:
            bad.append((d, kind, "zeval", [c for c in range(128) if ze[c] != want[c]]))
        assert [c for c in range(128) if want[c] == 0] == [c for c in range(128) if c not in present]
        want = [F.vanishing_inverse_on_coset_at_cell(z, c) for c in range(128)]
        zc = got.zcinv(d)
        if zc != want:
            bad.append((d, kind, "zcinv", [c for c in range(128) if zc[c] != want[c]]))
        if got.status[d] != 0:
            bad.append((d, kind, "status", got.status[d]))
        if got.coeff_bytes(d) != b"".join(F.fr_be(x) for x in POLYS[name]):
            bad.append((d, kind, "coeffs of " + name))
    assert not bad, "call %d: (missing, placement, stage, where) %s" % (call, bad[:20])


def test_both_sources(ctx):
    """the flat [R][128][2048] source, absent cells full of 0xFF bytes (never read): every output as from the list form"""
    blobs, listed = _decode_erasures(ctx, 0)
    flat = rs_decode(ctx.handle, blobs, flat=True, junk=FF_CELL)
    assert flat.rc == 0 and listed.rc == 0
    assert flat.status == listed.status == [0] * 65 and flat.deg == listed.deg == list(range(65))
    for which, what in enumerate(("zp", "zeval", "zcinv", "coeffs")):
        assert flat.raw[which] == listed.raw[which], what


# ---- edge evaluations ----------------------------------------------------------------------------------------------------------------------
def test_edge_evaluations(ctx):
    """blobs whose EVALUATIONS are a single non-zero entry, or all r - 1, at 64 and at 127 present cells"""
    rng = random.Random("rs-decode edge")
    evals = {}
    for pos, val in ((0, 1), (63, R - 1), (64, 1), (4095, R - 1)):
        evals["single %d" % pos] = [val if i == pos else 0 for i in range(4096)]
    evals["all r-1"] = [R - 1] * 4096
    blobs, want, names = [], [], []
    for name, ev in evals.items():
        coeffs = F.blob_to_coeffs(ev)
        cells = F.extend(coeffs)
        assert b"".join(cells[:64]) == b"".join(F.fr_be(x) for x in ev)  # cells 0 .. 63 are the blob
        if name == "all r-1":
            assert coeffs == [R - 1] + [0] * 4095
            half, one_gone = sorted(rng.sample(range(128), 64)), 77
        else:
            pos = int(name.split()[1])
            half, one_gone = list(range(64, 128)), pos // 64  # the non-zero entry is among the missing: in no cell at all / in the one missing cell
        for present in (half, [c for c in range(128) if c != one_gone]):
            blobs.append((present, cells))
            want.append(coeffs)
            names.append((name, len(present)))
    assert [n for _, n in names] == [64, 127] * 5
    got = rs_decode(ctx.handle, blobs)
    assert got.rc == 0 and got.status == [0] * 10 and got.deg == [64, 1] * 5
    for r, name in enumerate(names):
        assert got.coeffs(r) == want[r], name


# ---- inconsistency ---------------------------------------------------------------------------------------------------------------------------
def test_inconsistency_from_a_single_coefficient(ctx):
    """all 128 cells of a polynomial of degree >= 4096 with ONE non-zero high coefficient: status 4; the blobs next to it untouched"""
    low = _random_poly("rs-decode low half")
    highs = [(4096, 1), (6143, R - 1), (8191, random.Random("rs-decode high").randrange(1, R))]
    everything = list(range(128))
    good = [("random a", everything), ("all r-1", [c for c in range(128) if c % 5]), ("random b", list(range(1, 128, 2))), ("x^4095", everything)]
    blobs, want = [], []
    for k in range(7):
        if k % 2 == 0:
            name, present = good[k // 2]
            blobs.append((present, cells_of(name)))
            want.append(POLYS[name])
        else:
            at, val = highs[k // 2]
            blobs.append((everything, F.extend(low + [val if i == at else 0 for i in range(4096, at + 1)])))
            want.append(None)
    got = rs_decode(ctx.handle, blobs)
    assert got.rc == 0 and got.status == [0, 4, 0, 4, 0, 4, 0], got.status
    for r, w in enumerate(want):
        if w is not None:
            assert got.coeffs(r) == w, r


def test_a_foreign_cell_is_refused_where_the_oracle_refuses(ctx, oracle):
    """64 < present < 128 and one cell replaced by another polynomial's: status 4 exactly where the CPU oracle also refuses"""
    rng = random.Random("rs-decode foreign")
    mine, other = cells_of("random a"), cells_of("random b")
    blobs, names = [], []
    for n_present in (65, 100, 127):
        present = sorted(rng.sample(range(128), n_present))
        swap = present[rng.randrange(n_present)]
        tampered = dict(enumerate(mine))
        tampered[swap] = other[swap]
        blobs += [(present, tampered), (present, dict(enumerate(mine)))]
        names += [(n_present, "foreign cell %d" % swap), (n_present, "untouched")]
    refused = []
    for present, cells in blobs:
        try:
            oracle.recover_cells_and_kzg_proofs(present, [cells[c] for c in present])
            refused.append(False)
        except OracleError:
            refused.append(True)
    assert refused == [True, False] * 3, list(zip(names, refused))
    got = rs_decode(ctx.handle, blobs)
    assert got.rc == 0
    assert [s == 4 for s in got.status] == refused and all(s in (0, 4) for s in got.status), list(zip(names, got.status))
    for r in (1, 3, 5):
        assert got.coeffs(r) == POLYS["random a"], names[r]


# ---- non-canonical input -----------------------------------------------------------------------------------------------------------------------
def _with_element(cell, e, value):
    return cell[:32 * e] + value.to_bytes(32, "big") + cell[32 * (e + 1):]


def test_non_canonical_elements(ctx):
    """an element equal to r, or to 2^256 - 1, in a PRESENT cell: status 1 for that blob alone; in an ABSENT cell of the flat form: never read"""
    base = cells_of("random a")
    present = [c for c in range(128) if c % 3]  # 85 cells
    absent = [c for c in range(128) if c % 3 == 0]
    bad_r, bad_ff = dict(enumerate(base)), dict(enumerate(base))
    bad_r[present[0]] = _with_element(base[present[0]], 0, R)
    bad_ff[present[-1]] = _with_element(base[present[-1]], 63, 2 ** 256 - 1)
    blobs = [(present, dict(enumerate(cells_of("random b")))), (present, bad_r), (present, bad_ff), (present, dict(enumerate(base)))]
    for flat in (False, True):
        got = rs_decode(ctx.handle, blobs, flat=flat)
        assert got.rc == 0 and got.status == [0, 1, 1, 0], (flat, got.status)
        assert got.coeffs(0) == POLYS["random b"] and got.coeffs(3) == POLYS["random a"], flat
    # the same bytes where no cell is present: zeros around them, so that nothing else could explain a refusal
    zero = b"\0" * CELL
    junk = [{}, {absent[0]: _with_element(zero, 0, R)}, {absent[-1]: _with_element(zero, 63, 2 ** 256 - 1)}, {c: zero for c in absent}]
    for j in junk:
        for c in absent:
            j.setdefault(c, zero)
    clean = [(present, dict(enumerate(cells_of("random b"))))] + [(present, dict(enumerate(base)))] * 3
    got = rs_decode(ctx.handle, clean, flat=True, junk=junk)
    assert got.rc == 0 and got.status == [0, 0, 0, 0], got.status
    assert got.coeffs(0) == POLYS["random b"] and all(got.coeffs(r) == POLYS["random a"] for r in (1, 2, 3))


# ---- refused counts ----------------------------------------------------------------------------------------------------------------------------
def test_refused_counts(ctx):
    cells = dict(enumerate(cells_of("seven")))
    ok = (list(range(64)), cells)
    cases = {
        "63 cells": ([(list(range(63)), cells)], None),
        "129 cells": ([(list(range(128)), cells)], [129]),
        "descending indices": ([(list(range(64))[::-1], cells)], None),
        "equal indices": ([([5, 5] + list(range(6, 68)), cells)], None),
        "an index of 128": ([(list(range(63)) + [128], {**cells, 128: cells[0]})], None),
        "a good blob in front of 63 cells": ([ok, (list(range(1, 64)), cells)], None),
    }
    for name, (blobs, counts) in cases.items():
        for flat in (False, True):
            got = rs_decode(ctx.handle, blobs, flat=flat, counts=counts)
            assert got.rc == 3, (name, flat, got.rc)
            assert got.status == [-1] * got.n and got.deg == [-1] * got.n and not any(got.raw[3]), name  # nothing ran, nothing was written
    got = rs_decode(ctx.handle, [ok])  # and the context still decodes
    assert got.rc == 0 and got.status == [0] and got.deg == [64] and got.coeffs(0) == POLYS["seven"]
