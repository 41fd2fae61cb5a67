"""Every field and point operation of the kernels, one at a time, against exact integers (csrc/k_test_ops.hip, tests/device_ops.py).

Host leg: the host pass of every HD operation (no GPU).  It proves the case generator and the reference right before any GPU run.
GPU leg: the same cases through the device compilation -- fp30_mac.hpp's and fp29_mac.hpp's multiply-add chains, the slow paths as
real calls through their word buffers -- which must also give the host pass's words digit for digit; then the pair and quad forms
and the tree folds, which exist on the device only, in the callers' wave layouts.  Each result is checked for its value and for the
bound its type declares."""
import importlib
import os
import random

import pytest

import device_ops as D

kzg = importlib.import_module("rust-eth-kzg_amd")


def _lib_and_table():
    lib = kzg.load_library()
    if not hasattr(lib, "eth_kzg_amd_test_op"):
        pytest.fail("the test hooks library (libc_eth_kzg_hooks.so) is not the library loaded")
    return lib, D.op_table(lib)


def _hd_ops():
    return [n for n in D.SPEC]


_POINTS = None


def _points():
    global _POINTS
    if _POINTS is None:
        _POINTS = D._points(random.Random(D.POINT_POOL_SEED), 12)
    return _POINTS


def _cases(name):
    rng = random.Random("device-ops:" + name)
    ins = D.SPEC[name][0]
    if any(isinstance(t, D.Point) for t in ins):
        return D.point_cases(name, rng, _points())[0]
    return D.field_cases(name, rng)


def _check_all(name, cases, out):
    bad = []
    for i, (c, r) in enumerate(zip(cases, out)):
        e = D.check(name, c, [int(x) for x in r])
        if e:
            bad.append((i, e))
    assert not bad, f"{name}: {len(bad)} of {len(cases)} cases wrong, first: {bad[:3]}"


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_reference_group_law_matches_the_oracle():
    """The affine group law of device_ops.py against the oracle's scalar multiplication and MSM: multiples of the generator,
    a sum of multiples, the identity and a point minus itself."""
    import oracle_lib
    g = D.compress(D.G)
    for k in (1, 2, 3, 5, 255, 2 ** 64 + 7, D.R_ORDER - 1, 0x1234567890ABCDEF1234567890ABCDEF):
        assert D.compress(D.g_mul(D.G, k)) == oracle_lib.g1_mul(g, k.to_bytes(32, "big")), k
    ks = [11, 222, 3333, D.R_ORDER - 5]
    pts = [D.g_mul(D.G, 7 * i + 1) for i in range(len(ks))]
    want = None
    for a, k in zip(pts, ks):
        want = D.g_add(want, D.g_mul(a, k))
    got = oracle_lib.g1_msm(b"".join(D.compress(a) for a in pts), b"".join(k.to_bytes(32, "big") for k in ks))
    assert D.compress(want) == got
    a = D.g_mul(D.G, 99)
    assert D.g_add(a, D.g_neg(a)) is None and D.g_mul(D.G, D.R_ORDER) is None
    assert D.g_add(a, a) == D.g_mul(D.G, 198) and D.on_curve(a)


def test_every_spec_names_an_operation_of_the_library():
    lib, table = _lib_and_table()
    names = set(D.SPEC) | set(D.COOP) | set(D.FOLDS)
    assert names == set(table), (names ^ set(table))
    for n, (_, iw, ow, dev) in table.items():
        assert dev == (n in D.COOP or n in D.FOLDS), n
        if n in D.SPEC:
            ins, outs, _ = D.SPEC[n]
            assert (sum(t.words for t in ins), sum(t.words for t in outs)) == (iw, ow), n
    # the device-only forms have no host pass
    import numpy as np
    buf = np.zeros(table["coop4_add"][1], dtype=np.int32)
    out = np.zeros(table["coop4_add"][2], dtype=np.int32)
    assert lib.eth_kzg_amd_test_op(None, table["coop4_add"][0], 1, buf.ctypes.data, out.ctypes.data, 0) != 0


# ---- host leg ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _hd_ops())
def test_host_pass_matches_exact_integers(name):
    lib, table = _lib_and_table()
    cases = _cases(name)
    assert len(cases) >= 8
    out = D.run(lib, table, name, cases)
    _check_all(name, cases, out)


# ---- GPU leg ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_ctx():
    """a context with the smallest tables: these operations do not read them"""
    import torch
    torch.cuda.init()
    saved = os.environ.get("ETH_KZG_AMD_TABLE_GB")
    os.environ["ETH_KZG_AMD_TABLE_GB"] = "3"
    try:
        c = kzg.DASContext(use_precomp=True)
    finally:
        if saved is None:
            os.environ.pop("ETH_KZG_AMD_TABLE_GB", None)
        else:
            os.environ["ETH_KZG_AMD_TABLE_GB"] = saved
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", _hd_ops())
def test_device_matches_exact_integers_and_the_host_pass(small_ctx, name):
    import numpy as np
    lib, table = _lib_and_table()
    cases = _cases(name)
    dev = D.run(lib, table, name, cases, small_ctx.handle, on_device=True)
    _check_all(name, cases, dev)
    host = D.run(lib, table, name, cases)
    diff = np.nonzero((dev != host).any(axis=1))[0]
    assert diff.size == 0, f"{name}: device words differ from the host pass in {diff.size} cases, first {diff[:5].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(D.COOP))
def test_pair_and_quad_forms_in_wave_layouts(small_ctx, name):
    """Every lane of the group ends with the whole, right result; exceptional operations next to regular ones in the same wave."""
    lib, table = _lib_and_table()
    base, co = D.COOP[name]
    rng = random.Random("device-ops:" + name)
    cases = D.coop_cases(name, rng, _points())
    assert len(cases) % (64 // co) != 0
    out = D.run(lib, table, name, cases, small_ctx.handle, on_device=True)
    ow = table[name][2] // co
    bad = []
    for i, (c, r) in enumerate(zip(cases, out)):
        copies = [list(r[k * ow:(k + 1) * ow]) for k in range(co)]
        if any(x != copies[0] for x in copies[1:]):
            bad.append((i, "lanes of the group disagree"))
            continue
        r0 = [int(x) for x in copies[0]]
        if name == "coop4_dbl_half_phi":  # the doubling, and beta X of the operand in the lane the first level leaves idle
            e = D.check("jacs_dbl_half", c[:39], r0[:39])
            if not e and D.Fs(1, D.DC, True).bound_error(r0[39:]):
                e = "beta x: bound"
            if not e and D.Fs(1, D.DC).residue(r0[39:]) != D.JACS.coords[0].residue(c[:13]) * D.BETA % D.P:
                e = "beta x: value"
        else:
            e = D.check(base, c, r0)
        if e:
            bad.append((i, e))
    assert not bad, f"{name}: {len(bad)} of {len(cases)} operations wrong, first: {bad[:3]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(D.FOLDS))
def test_tree_folds_with_identities_and_equal_partial_sums(small_ctx, name):
    lib, table = _lib_and_table()
    pt, nt = D.FOLDS[name]
    rng = random.Random("device-ops:" + name)
    cases, refs = D.fold_cases(name, rng, _points())
    out = D.run(lib, table, name, cases, small_ctx.handle, on_device=True)
    for i, (r, want) in enumerate(zip(out, refs)):
        r = [int(x) for x in r]
        assert pt.bound_error(r) is None, (name, i, pt.bound_error(r))
        assert pt.affine(r) == want, (name, i)
