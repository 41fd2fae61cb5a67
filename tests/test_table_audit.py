"""Every entry of the fixed-base window tables against exact integers.

The library's audit (csrc/table_audit.hpp behind include/c_eth_kzg_test_hooks.h) decides per entry: canonical encoding, on the curve,
T[d] = T[d-1] + T[1] by a collinearity / tangent test with the degenerate cases excluded, the first entry of a window = 2^bits times the
first entry of the window below, the first entry of window 0 = the base, identity rows all zero and no zero entry elsewhere.  By
induction a row without findings is d 2^lo(w) B for every d.

Host leg (no GPU): synthetic tables built here from plain integers (widths 8 and 12: mixed window widths, both blocks of a group, an
identity base) must pass with exactly the computed number of visits, and every planted fault must be reported at its place and
nowhere else.  Where a finding may appear: an altered entry e = (row, d) can break the relations that involve it -- its own checks and
the step of d + 1 -- so the findings must lie in the union of {d, d + 1} over the altered entries, plus {1, 2} of the same base in the
window above when d = 1 (the link); every altered entry must itself be reported (behind a broken head of the row, d = 1 or 2, only
the head: the audit does not repeat a wrong first entry at every d of its row).  The same tables go through the Python predicate
(tests/device_ops.py: audit_row), which must agree reason for reason.

GPU leg: the device pass reports what the host pass reports on the synthetic tables; then the real tables of contexts in every
configuration that builds them differently: zero findings, every entry visited (count == groups x bases x entries per base, x 96 bytes
== the table's payload), the first entry of window 0 of EVERY (group, base) equal to the oracle's base, and -- the audit itself against
Python -- whole rows read back and put through audit_row and through the direct statement d 2^lo B (row_multiples_error), plus every
entry that begins or ends a table piece.

The row sample (measured on the development machine: 47 us per entry for both Python checks, 1.5 s per row of 32768): per table
SAMPLES[.][0] rows in the first and as many in the last group, their windows cycling through all W (both blocks of a group),
and for up to SAMPLES[.][1] boundaries between two launches of the builder (groups that share its scratch) one row in the last
group of the chunk and one in the first of the next.  "full" (the two table budgets): 8 + 8 + 2 x 4 = 24 rows per table, about 50 s of
Python for the 206 + 35 GB pair; "light" (every other configuration): 3 + 3 + 2 x 2 = 10 rows."""
import ctypes as C
import importlib
import os
import random
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import device_ops as D
import oracle_lib
import setup_material as sm
import synth
from conftest import TABLE_BUDGETS, table_budget_ctx

kzg = importlib.import_module("rust-eth-kzg_amd")
INF = b"\xc0" + bytes(47)
MAX_FINDINGS = 256
FK, SRS = 0, 1
MAIN, NEXT, START = 0, 1, 2
SAMPLES = {"full": (8, 4), "light": (3, 2)}  # rows per edge group, builder-chunk boundaries


# ---- the hooks -------------------------------------------------------------------------------------------------------------------
def _findings(buf, n):
    return [tuple(int(x) for x in buf[k]) for k in range(min(n, len(buf)))]


def audit_buffer(table, bases, c, n_groups, nb, handle=None, on_device=False):
    """(visited, n_findings, [(group, window, base, d, reasons)]) of a caller's table: np.uint32 [entries, 24], bases [(x, y) | None]"""
    lib = kzg.load_library()
    t = np.ascontiguousarray(table, dtype=np.uint32)
    b = np.array([D.g1affine_words(a) for a in bases], dtype=np.uint32)
    visited, n = C.c_uint64(0), C.c_uint64(0)
    f = np.zeros((MAX_FINDINGS, 5), dtype=np.int32)
    rc = lib.eth_kzg_amd_test_table_audit_buffer(handle, c, n_groups, nb, t.ctypes.data, b.ctypes.data, int(on_device), C.byref(visited),
                                                 C.byref(n), f.ctypes.data, MAX_FINDINGS)
    assert rc == 0, rc
    return visited.value, n.value, _findings(f, n.value)


def table_info(ctx, kind, which):
    """None if there is no such table, else its shape, payload bytes, builder chunk and the first block of every piece"""
    lib = kzg.load_library()
    out = np.zeros(8, dtype=np.int64)
    pieces = np.zeros(512, dtype=np.int32)
    if lib.eth_kzg_amd_test_table_info(ctx.handle, kind, which, out.ctypes.data, pieces.ctypes.data, len(pieces)) != 0:
        return None
    keys = ("c", "n_groups", "nb", "state", "ready", "bytes", "chunk", "n_pieces")
    info = dict(zip(keys, (int(x) for x in out)))
    assert info["n_pieces"] <= len(pieces)
    info["piece_first_block"] = [int(x) for x in pieces[:info["n_pieces"]]]
    return info


def table_audit(ctx, kind, which):
    lib = kzg.load_library()
    visited, n, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
    f = np.zeros((MAX_FINDINGS, 5), dtype=np.int32)
    t0 = time.perf_counter()
    rc = lib.eth_kzg_amd_test_table_audit(ctx.handle, kind, which, C.byref(visited), C.byref(n), f.ctypes.data, MAX_FINDINGS, C.byref(ms))
    wall = (time.perf_counter() - t0) * 1e3
    assert rc == 0, rc
    return visited.value, n.value, _findings(f, n.value), ms.value, wall


def table_read(ctx, kind, which, group, w, i, d0, n):
    lib = kzg.load_library()
    out = np.zeros((n, 24), dtype=np.uint32)
    rc = lib.eth_kzg_amd_test_table_read(ctx.handle, kind, which, group, w, i, d0, n, out.ctypes.data)
    assert rc == 0, (rc, kind, which, group, w, i, d0, n)
    return out


# ---- synthetic tables from exact integers ----------------------------------------------------------------------------------------
N_GROUPS, NB = 2, 2
_SYNTH = {}


def synth_table(c):
    """two groups of two bases, base 1 of group 1 the identity: (words [entries, 24], bases)"""
    if c not in _SYNTH:
        rng = random.Random(1000 + c)
        bases = [D.g_mul(D.G, rng.randrange(1, D.R_ORDER)) for _ in range(N_GROUPS * NB)]
        bases[1 * NB + 1] = None
        t = np.zeros((D.glv_table_entries(c, N_GROUPS, NB), 24), dtype=np.uint32)
        for g in range(N_GROUPS):
            for i in range(NB):
                q = bases[g * NB + i]
                for w in range(D.glv_windows(c)):
                    bits = D.glv_window_bits(c, w)
                    at = D.glv_entry_index(c, NB, g, w, i, 1)
                    cur = None
                    for d in range(1, (1 << (bits - 1)) + 1):
                        cur = D.g_add(cur, q)
                        t[at + d - 1] = D.tabs_pack(cur)
                    for _ in range(bits):
                        q = D.g_add(q, q)
        _SYNTH[c] = (t, bases)
    t, bases = _SYNTH[c]
    return t.copy(), list(bases)


def _at(c, g, w, i, d):
    return D.glv_entry_index(c, NB, g, w, i, d)


def _T(c, w):
    return 1 << (D.glv_window_bits(c, w) - 1)


def _repack(words, fx=lambda v: v, fy=lambda v: v):
    return D.tabs_pack_value(fx(D.tabs_unpack_value(words[:12]))) + D.tabs_pack_value(fy(D.tabs_unpack_value(words[12:])))


# each fault: (table, c, g, w, i, d) -> the entries it altered
def f_digit_off_by_one(t, c, g, w, i, d):
    k = 3 + d % 7 + 12 * (d & 1)  # some digit of x or y
    x = int(t[_at(c, g, w, i, d), k])
    t[_at(c, g, w, i, d), k] = (x & 0xC0000000) | ((x + 1) & 0x3FFFFFFF)
    return [(g, w, i, d)]


def f_non_canonical_digits(t, c, g, w, i, d):
    e = _at(c, g, w, i, d)
    t[e] = _repack(t[e], fx=lambda v: v + D.P) if d & 1 else _repack(t[e], fy=lambda v: v + D.P)
    return [(g, w, i, d)]


def f_y_negated(t, c, g, w, i, d):
    e = _at(c, g, w, i, d)
    t[e] = _repack(t[e], fy=lambda v: (D.P - v) % D.P)
    return [(g, w, i, d)]


def f_neighbours_swapped(t, c, g, w, i, d):
    if d == _T(c, w):
        d -= 1
    a, b = _at(c, g, w, i, d), _at(c, g, w, i, d + 1)
    t[[a, b]] = t[[b, a]]
    return [(g, w, i, d), (g, w, i, d + 1)]


def f_other_base(t, c, g, w, i, d):
    t[_at(c, g, w, i, d)] = t[_at(c, g, w, 1 - i, d)]
    return [(g, w, i, d)]


def f_lane_step_slip(t, c, g, w, i, d):
    src = d + 64 if d + 64 <= _T(c, w) else d - 64  # the last entries of a row have nothing 64 above them: the slip the other way
    t[_at(c, g, w, i, d)] = t[_at(c, g, w, i, src)]
    return [(g, w, i, d)]


def f_zero_entry(t, c, g, w, i, d):
    t[_at(c, g, w, i, d)] = 0
    return [(g, w, i, d)]


def f_first_entry_doubled(t, c, g, w, i, d):
    e = _at(c, g, w, i, 1)
    p = D.tabs_point(t[e])
    t[e] = D.tabs_pack(D.g_add(p, p))
    return [(g, w, i, 1)]


ROW_FAULTS = [f_digit_off_by_one, f_non_canonical_digits, f_y_negated, f_neighbours_swapped, f_other_base, f_lane_step_slip, f_zero_entry]
REASON_OF = {f_digit_off_by_one: D.A_OFF_CURVE, f_non_canonical_digits: D.A_ENCODING, f_zero_entry: D.A_ZERO}


def allowed_places(c, altered):
    out = set()
    for (g, w, i, d) in altered:
        out.add((g, w, i, d))
        if d + 1 <= _T(c, w):
            out.add((g, w, i, d + 1))
        if d == 1 and w + 1 < D.glv_windows(c):
            out |= {(g, w + 1, i, 1), (g, w + 1, i, 2)}
    return out


def plant_cases(c):
    """(name, fault, g, w, i, d): in group 0 (both bases live) a wide window of the lower block and the narrowest, last window of the
    upper block; d = first, second, interior, 64, 65, last"""
    W = D.glv_windows(c)
    cases = []
    for w in (0, W - 1):
        T = _T(c, w)
        for d in (1, 2, 37, 64, 65, T - 1, T):
            for f in ROW_FAULTS:
                cases.append((f"{f.__name__[2:]}-w{w}-d{d}", f, 0, w, d % 2, d))
    for w in (0, W // 2, W - 1):  # a first entry doubled once too often: lower block, across the block split, last window
        cases.append((f"first_entry_doubled-w{w}", f_first_entry_doubled, 0, w, 0, 1))
        cases.append((f"first_entry_doubled-g1-w{w}", f_first_entry_doubled, 1, w, 0, 1))
    for w in (0, W - 1):  # a non-zero entry in the identity row of group 1
        for d in (1, 64, 65, _T(c, w)):
            cases.append((f"nonzero_in_identity_row-w{w}-d{d}", None, 1, w, 1, d))
    return cases


def python_findings(t, bases, c, rows):
    """audit_row over the rows [(g, w, i)]: {(g, w, i, d): reasons}"""
    out = {}
    for (g, w, i) in sorted(set(rows)):
        T = _T(c, w)
        row = t[_at(c, g, w, i, 1):_at(c, g, w, i, 1) + T]
        prev = t[_at(c, g, w - 1, i, 1)] if w else None
        r = D.audit_row(row, D.glv_window_bits(c, w - 1) if w else 0, prev, bases[g * NB + i], identity_row=bases[g * NB + i] is None)
        out.update({(g, w, i, d): v for d, v in r.items()})
    return out


def run_plant(c, case, audit):
    name, fault, g, w, i, d = case
    t, bases = synth_table(c)
    if fault is None:
        t[_at(c, g, w, i, d)] = t[_at(c, 0, w, 0, d)]
        altered, allowed = [(g, w, i, d)], {(g, w, i, d)}
    else:
        altered = fault(t, c, g, w, i, d)
        allowed = allowed_places(c, altered)
    visited, n, found = audit(t, bases)
    assert visited == D.glv_table_entries(c, N_GROUPS, NB), (name, visited)
    assert n == len(found), (name, n)
    places = {f[:4] for f in found}
    assert places, f"{name}: the planted fault passed the audit"
    assert places <= allowed, (name, sorted(places - allowed))
    # every altered entry is itself reported -- except that behind a broken head of the row (d = 1, 2 altered, and reported) the steps of
    # d >= 3 stay silent (csrc/table_audit.hpp)
    head_broken = any(e[3] <= 2 for e in altered)
    must = {e for e in altered if e[3] <= 2 or not head_broken}
    assert must <= places, (name, "an altered entry is not reported", sorted(must - places))
    reasons = {f[:4]: f[4] for f in found}
    if fault in REASON_OF:
        assert reasons[altered[0]] & REASON_OF[fault], (name, reasons)
    if fault is f_non_canonical_digits:
        assert reasons == {altered[0]: D.A_ENCODING}, (name, reasons)  # the residue is right: nothing else may see it
    if fault is None:
        assert reasons == {altered[0]: D.A_NONZERO_IDENTITY}, (name, reasons)
    return t, bases, altered, reasons


def host_audit(c):
    return lambda t, bases: audit_buffer(t, bases, c, N_GROUPS, NB)


# ---- host leg --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [8, 12])
def test_host_clean_synthetic_table_has_no_findings_and_every_entry_is_visited(c):
    t, bases = synth_table(c)
    W = D.glv_windows(c)
    assert {D.glv_window_bits(c, w) for w in range(W)} == ({8} if c == 8 else {12, 11}), "width 12 has mixed window widths"
    assert sum(D.glv_window_bits(c, w) for w in range(W)) == 128
    visited, n, found = audit_buffer(t, bases, c, N_GROUPS, NB)
    assert (n, found) == (0, [])
    assert visited == N_GROUPS * NB * D.glv_entries_per_base(c) == len(t)
    # the Python predicate on the same table: every row, nothing found; and the rows are the multiples they should be
    rows = [(g, w, i) for g in range(N_GROUPS) for i in range(NB) for w in (range(W) if c == 8 else (0, W // 2, W - 1))]
    assert python_findings(t, bases, c, rows) == {}
    for (g, w, i) in rows:
        if bases[g * NB + i] is not None:
            q = D.g_mul(bases[g * NB + i], 1 << D.glv_window_lo(c, w))
            assert D.row_multiples_error(t[_at(c, g, w, i, 1):_at(c, g, w, i, 1) + _T(c, w)], q) is None, (g, w, i)


@pytest.mark.parametrize("c", [8, 12])
def test_host_every_planted_fault_is_reported_at_its_place(c):
    for case in plant_cases(c):
        t, bases, altered, reasons = run_plant(c, case, host_audit(c))
        # the Python predicate on the rows involved: the same findings, reason for reason
        rows = {(g, w, i) for (g, w, i, d) in altered} | {(g, w + 1, i) for (g, w, i, d) in altered if d == 1 and w + 1 < D.glv_windows(c)}
        assert python_findings(t, bases, c, rows) == reasons, case[0]


def test_host_more_findings_than_the_buffer_holds_are_counted():
    c = 8
    t, bases = synth_table(c)
    t[_at(c, 0, 3, 0, 1):_at(c, 0, 3, 0, 1) + 128] = 0  # a whole live row zeroed
    t[_at(c, 0, 4, 1, 1):_at(c, 0, 4, 1, 1) + 128] = 0
    visited, n, found = audit_buffer(t, bases, c, N_GROUPS, NB)
    assert visited == len(t) and n >= 256 and len(found) == MAX_FINDINGS
    assert found == sorted(found)


def test_packer_matches_the_device_packing():
    """tabs_pack (this reference) against tabs_pack_coord / tabs_unpack of curve30.hpp through the per-operation hook"""
    lib = kzg.load_library()
    table = D.op_table(lib)
    rng = random.Random(5)
    pts = [D.g_mul(D.G, rng.randrange(1, D.R_ORDER)) for _ in range(8)]
    cases = [D.fs_digits(a[0] * D.RS % D.P, D.DU) + D.fs_digits(a[1] * D.RS % D.P, D.DU) for a in pts]
    out = D.run(lib, table, "fs_tabs_pack_unpack", cases)
    for a, o in zip(pts, out):
        words = [int(x) & 0xFFFFFFFF for x in o[:24]]
        assert words == D.tabs_pack(a) and D.tabs_point(words) == a


# ---- GPU leg: the synthetic tables ---------------------------------------------------------------------------------------------------
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def small_ctx():
    _torch_first()
    c = kzg.DASContext(use_precomp=False)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("c", [8, 12])
def test_device_pass_reports_what_the_host_pass_reports(small_ctx, c):
    t, bases = synth_table(c)
    assert audit_buffer(t, bases, c, N_GROUPS, NB, small_ctx.handle, True) == audit_buffer(t, bases, c, N_GROUPS, NB) == (len(t), 0, [])
    for case in plant_cases(c):
        t, bases, altered, reasons = run_plant(c, case, lambda tt, bb: audit_buffer(tt, bb, c, N_GROUPS, NB, small_ctx.handle, True))
        assert audit_buffer(t, bases, c, N_GROUPS, NB, small_ctx.handle, True) == audit_buffer(t, bases, c, N_GROUPS, NB), case[0]


# ---- GPU leg: the real tables ----------------------------------------------------------------------------------------------------------
def fk20_bases(g1=None):
    """[group j][base i] -> 48 bytes: FFT_128 of SRS vector i (batch_toeplitz.rs:46-61) by the oracle; mainnet: test_gpu_fullsize's"""
    if g1 is None:
        import test_gpu_fullsize as full
        cols = [full._fk20_base_column(i) for i in range(64)]
    else:
        srs = [g1[48 * k:48 * (k + 1)] for k in range(4096)]
        cols = []
        for i in range(64):
            vec = [srs[4096 - 1 - 64 - (i + 64 * pos)] if pos < 63 else INF for pos in range(128)]
            out = oracle_lib.g1_fft(b"".join(vec), inverse=False)
            cols.append([out[48 * j:48 * (j + 1)] for j in range(128)])
    return [[cols[i][j] for i in range(64)] for j in range(128)]


def srs_bases(g1=None):
    g1 = sm.mainnet_points()[0] if g1 is None else g1
    return [[g1[48 * (64 * g + i):48 * (64 * g + i + 1)] for i in range(64)] for g in range(64)]


def _spread(n, k):
    return sorted({(n - 1) * j // max(1, k - 1) for j in range(k)}) if n > 1 else [0]


def sample_rows(info, sample):
    """[(group, window, base)]: the module docstring's sample"""
    per_edge, n_bound = SAMPLES[sample]
    G, nb, W, chunk = info["n_groups"], info["nb"], D.glv_windows(info["c"]), info["chunk"]
    rows = []
    for e, g in enumerate((0, G - 1)):
        for k in range(per_edge):
            rows.append((g, (k + e * (W // 2)) % W, (7 + 23 * k + 31 * e) % nb))
    if chunk and chunk < G:
        bounds = list(range(chunk, G, chunk))  # first group of every launch but the first
        for k, b in enumerate(bounds[j] for j in _spread(len(bounds), n_bound)):
            rows += [(b - 1, (W - 1 - k) % W, (11 + 17 * k) % nb), (b, (W // 2 + k) % W, (5 + 29 * k) % nb)]
    return sorted(set(rows))


def audit_real_table(ctx, kind, which, want_bases, sample, tag):
    """one table of a context: the device audit, then the audit against Python.  Returns its info + the audit's times."""
    info = table_info(ctx, kind, which)
    assert info is not None, (tag, kind, which)
    c, G, nb = info["c"], info["n_groups"], info["nb"]
    W, WL = D.glv_windows(c), D.glv_lower_windows(c)
    assert (G, nb) == ((128, 64) if kind == FK else (64, 64)) and info["state"] == 1 and info["ready"] == G, (tag, info)
    visited, n, found, ms, wall = table_audit(ctx, kind, which)
    print(f"table-audit {tag} kind={'fk20' if kind == FK else 'commitment'} width={c} bytes={info['bytes']} entries={visited} "
          f"kernel_ms={ms:.1f} wall_ms={wall:.1f} chunk={info['chunk']} pieces={info['n_pieces']}")
    assert (n, found) == (0, []), (tag, kind, n, found[:8])
    assert visited == G * nb * D.glv_entries_per_base(c), (tag, kind, visited)  # the share of entries the audit may skip is zero
    assert visited * 96 == info["bytes"], (tag, kind, visited, info["bytes"])
    # the induction's anchor: entry d = 1 of window 0 of every (group, base) is the oracle's base
    anchor = {}
    for g in range(G):
        for i in range(nb):
            p = D.tabs_point(table_read(ctx, kind, which, g, 0, i, 1, 1)[0])
            assert p is not None and D.compress(p) == want_bases[g][i] and D.on_curve(p), (tag, kind, g, i)
            anchor[(g, i)] = p
    # whole rows through the Python predicate and the direct statement
    t0 = time.perf_counter()
    rows = sample_rows(info, sample)
    assert {w >= WL for (_, w, _) in rows} == {False, True}, "both blocks of a group"
    n_entries = 0
    for (g, w, i) in rows:
        T = 1 << (D.glv_window_bits(c, w) - 1)
        row = table_read(ctx, kind, which, g, w, i, 1, T)
        prev = table_read(ctx, kind, which, g, w - 1, i, 1, 1)[0] if w else None
        assert D.audit_row(row, D.glv_window_bits(c, w - 1) if w else 0, prev, anchor[(g, i)]) == {}, (tag, kind, g, w, i)
        q = D.g_mul(anchor[(g, i)], 1 << D.glv_window_lo(c, w))
        assert D.row_multiples_error(row, q) is None, (tag, kind, g, w, i)
        n_entries += T
    # every entry that begins or ends a table piece
    first = info["piece_first_block"]
    assert first and first[0] == 0 and first == sorted(set(first)) and first[-1] < 2 * G, (tag, first)
    for k, fb in enumerate(first):
        lb = (first[k + 1] if k + 1 < len(first) else 2 * G) - 1
        for (blk, w, i, d) in ((fb, WL * (fb & 1), 0, 1), (lb, W - 1 if lb & 1 else WL - 1, nb - 1, None)):
            d = d or 1 << (D.glv_window_bits(c, w) - 1)
            p = D.tabs_point(table_read(ctx, kind, which, blk // 2, w, i, d, 1)[0])
            assert p == D.g_mul(anchor[(blk // 2, i)], d << D.glv_window_lo(c, w)), (tag, kind, "piece", k, blk, w, i, d)
    print(f"table-audit {tag} kind={kind} python: {len(rows)} rows, {n_entries} entries, {2 * len(first)} piece edges in {time.perf_counter() - t0:.1f} s")
    return info


def audit_context(ctx, sample, tag, which=MAIN, fk=None, srs=None):
    infos = [audit_real_table(ctx, FK, which, fk or fk20_bases(), sample, tag), audit_real_table(ctx, SRS, which, srs or srs_bases(), sample, tag)]
    if which == MAIN:
        assert ctx.table_bytes() == sum(x["bytes"] for x in infos), (tag, ctx.table_bytes())
    return infos


@pytest.mark.gpu
@pytest.mark.parametrize("width", [14, 12, 8])
def test_tables_of_every_narrower_width(monkeypatch, width):
    _torch_first()
    monkeypatch.setenv("ETH_KZG_AMD_GLV_WINDOW", str(width))
    c = kzg.DASContext(use_precomp=True)
    try:
        assert c.window_bits() == width and c.tables_ready() == 1
        fk, srs = audit_context(c, "light", f"width-{width}")
        assert fk["c"] == width
    finally:
        c.close()


@pytest.mark.gpu
def test_tables_without_precomputation(small_ctx):
    fk, srs = audit_context(small_ctx, "light", "no-precomp")
    assert (fk["c"], srs["c"]) == (8, 8)


@pytest.mark.gpu
def test_start_tables_then_wide_tables_built_under_load(monkeypatch, oracle):
    """A progressive start: the start tables right after the constructor returns; the groups of the growing table that are already
    published, while the builder runs and this thread keeps calling compute_cells_and_kzg_proofs; the wide tables when it is done."""
    _torch_first()
    monkeypatch.delenv("ETH_KZG_AMD_TABLE_GB", raising=False)  # the default budget: nine windows each
    monkeypatch.delenv("ETH_KZG_AMD_PROGRESSIVE", raising=False)
    c = kzg.DASContext(use_precomp=True, wait_tables=False)
    try:
        start = [table_info(c, k, START) for k in (FK, SRS)]
        assert all(s is not None and s["c"] == 8 and s["state"] == 1 for s in start), start
        for kind in (FK, SRS):
            visited, n, found, ms, wall = table_audit(c, kind, START)
            assert (n, found) == (0, []) and visited == start[kind]["n_groups"] * 64 * D.glv_entries_per_base(8), (kind, n, visited)
            assert visited * 96 == start[kind]["bytes"]
        blob = synth.seeded_blob(4141)
        want = oracle.compute_cells_and_kzg_proofs(blob)
        calls, partial = 0, []
        while c.tables_ready(0) == 0:
            assert tuple(c.compute_cells_and_kzg_proofs(blob)) == want
            calls += 1
            if calls % 8 == 0:  # what the next MSM launch would take from the growing table: its ready groups, as they are now
                for kind in (FK, SRS):
                    nxt = table_info(c, kind, NEXT)
                    if nxt is not None and nxt["state"] == 0:
                        visited, n, found, ms, wall = table_audit(c, kind, NEXT)
                        assert (n, found) == (0, []), (kind, found[:8])
                        assert visited % (64 * D.glv_entries_per_base(nxt["c"])) == 0
                        groups = visited // (64 * D.glv_entries_per_base(nxt["c"]))
                        assert nxt["ready"] <= groups <= nxt["n_groups"], (kind, nxt["ready"], groups)
                        partial.append((kind, groups))
        print(f"table-audit under-load: {calls} calls while the builder ran, partial audits {partial}")
        assert c.tables_ready(-1) == 1 and calls >= 1
        assert tuple(c.compute_cells_and_kzg_proofs(blob)) == want
        fk, srs = audit_context(c, "light", "built-under-load")
        assert (fk["c"], srs["c"]) == (15, 15)
        assert fk["chunk"] == 1, "a progressive build fills one group per launch"
    finally:
        c.close()


@pytest.mark.gpu
def test_tables_of_a_custom_setup_next_to_a_live_mainnet_context(tmp_path_factory):
    _torch_first()
    g1, g2 = sm.insecure_setup(tmp_path_factory.getbasetemp())
    mainnet = kzg.DASContext(use_precomp=True, table_budget_gb=25)
    try:
        custom = kzg.DASContext.from_trusted_setup(g1, g2, use_precomp=True, table_budget_gb=25)
        try:
            assert custom.setup_digest != mainnet.setup_digest
            cfk, csrs = audit_context(custom, "light", "custom-setup", fk=fk20_bases(g1), srs=srs_bases(g1))
            mfk, msrs = audit_context(mainnet, "light", "mainnet-next-to-custom")
            assert (cfk["c"], csrs["c"]) == (mfk["c"], msrs["c"]) == (12, 12)
        finally:
            custom.close()
    finally:
        mainnet.close()


# last in the module: the module-scoped context of the wider budget holds 242 GB until the module ends
@pytest.fixture(scope="module", params=TABLE_BUDGETS, ids=["tables-" + b for b in TABLE_BUDGETS])
def budget_ctx(request):
    _torch_first()
    yield from table_budget_ctx(request.param, lambda: kzg.DASContext(use_precomp=True))


@pytest.mark.gpu
def test_tables_of_both_budgets(budget_ctx):
    fk, srs = audit_context(budget_ctx, "full", "budget")
    assert (fk["c"], srs["c"]) in ((15, 15), (16, 15))
    assert fk["chunk"] >= 1 and srs["chunk"] >= 1
