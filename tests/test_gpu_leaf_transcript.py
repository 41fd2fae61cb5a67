"""Cell verification with the leaf-hashed challenge (ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT): the leaf kernel, the root, the pairing inputs,
the error split and the reference's verdicts.

The statement of the transcript is tests/leaf_transcript.py (hashlib, written from the definition); the group arithmetic behind the
challenge is tests/verify_transcript.py's cell_partial, which takes the challenge as an argument and is reused unchanged.  Material and
contexts as tests/test_verify_inputs.py builds them: the six blobs of verify_transcript.material_blobs() and two contexts, one on the
windowed and one on the byte-shifted form of the lincombs at every batch size.

1. k_sha256_cell_leaves alone (eth_kzg_amd_test_cell_leaf_digests): n = 1, 2, 63, 64, 65, 129 -- one lane, a wave less one, a wave, a
   wave plus one, two waves plus one -- over entries that repeat commitments and hold the indices 0 and 127; every digest.
2. eth_kzg_amd_test_verify_cells_inputs_ex on ten cases of verify_transcript.cell_cases(): the root bytes and the 96 bytes of the two
   pairing inputs under the leaf challenge, the same under the reference's with flags = 0, both forms of the lincombs, the host form
   and (len-257) the device-resident form; the flagged public calls verify all of them.
3. Wrong proofs and malformed input: flagged and unflagged calls agree, host and device-resident form; n = 0; an unknown flag bit.
4. The 30 verify_cell_kzg_proof_batch cases of tests/golden/vectors.json through the flagged call."""
import ctypes as C
import importlib
import os
import random

import numpy as np
import pytest

import leaf_transcript as L
import vectors
import verify_transcript as T

kzg = importlib.import_module("rust-eth-kzg_amd")
pytestmark = pytest.mark.gpu

LEAF = 1  # ETH_KZG_AMD_VERIFY_LEAF_TRANSCRIPT
CASES = {c.name: c for c in T.cell_cases()}
INPUT_CASES = ["len-1", "len-2", "len-63", "len-64", "len-65", "len-257", "four-interleaved", "row-of-280-next-to-row-of-1", "one-index",
               "identity-commitment-mixed"]
DEVICE_CASES = ["len-257"]
LEAF_SIZES = [1, 2, 63, 64, 65, 129]
_statement = {}  # (case, flags) -> (root bytes, 96 bytes): computed once, shared by the forms, never changed


def _ctx(**env):
    import torch
    torch.cuda.init()
    env = dict(env, ETH_KZG_AMD_TABLE_GB="3")  # the start tables: results never depend on the table
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return kzg.DASContext(use_precomp=True)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def forms():
    c = {"windowed": _ctx(ETH_KZG_AMD_PIP_SHIFT_MIN=str(1 << 20)), "shifted": _ctx(ETH_KZG_AMD_PIP_SHIFT_MIN="1")}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def material(forms):
    ctx = forms["windowed"]
    blobs = T.material_blobs()
    st, cells, proofs = ctx.compute_cells_and_kzg_proofs_batch(blobs)
    assert st == [0] * len(blobs)
    comms = [ctx.blob_to_kzg_commitment(b) for b in blobs]
    return T.Material(blobs, comms, cells, proofs, [None] * len(blobs))


def _want(mat, case, flags):
    key = (case.name, flags)
    if key not in _statement:
        args = case.args(mat)
        root = L.leaf_root(*args) if flags else T.cell_digest(*args)
        _statement[key] = (root, T.cell_partial(*args, 0, len(args[1]), r=T.reduce_digest(root)))
    return _statement[key]


def _device_arrays(args):
    import torch
    comm, idx, cells, proofs = args
    dev = lambda raw: torch.frombuffer(bytearray(raw) or bytearray(1), dtype=torch.uint8).cuda()  # noqa: E731
    arrays = (dev(b"".join(comm)), torch.from_numpy(np.array(list(idx) or [0], dtype=np.int64)).cuda(), dev(b"".join(cells)), dev(b"".join(proofs)))
    torch.cuda.synchronize()
    return arrays


def _inputs_ex(ctx, args, flags, device_arrays=None):
    """eth_kzg_amd_test_verify_cells_inputs_ex -> (rc, root bytes, 96 bytes)"""
    lib = kzg.load_library()
    comm, idx, cells, proofs = args
    n = len(idx)
    root, out = C.create_string_buffer(32), C.create_string_buffer(96)
    if device_arrays is not None:
        d_c, d_i, d_l, d_p = device_arrays
        rc = lib.eth_kzg_amd_test_verify_cells_inputs_ex(ctx.handle, n, 1, d_c.data_ptr(), d_i.data_ptr(), d_l.data_ptr(), d_p.data_ptr(), flags, root, out)
    else:
        ca, _k1 = kzg._flat_ptrs(comm, 48)
        la, _k2 = kzg._flat_ptrs(cells, 2048)
        pa, _k3 = kzg._flat_ptrs(proofs, 48)
        ia = np.array(idx, dtype=np.uint64)
        rc = lib.eth_kzg_amd_test_verify_cells_inputs_ex(ctx.handle, n, 0, kzg._vp(ca), kzg._vp(ia), kzg._vp(la), kzg._vp(pa), flags, root, out)
    return rc, root.raw, out.raw


# ---- 1. the leaf kernel alone ----------------------------------------------------------------------------------------------------------
def _leaf_entries():
    """129 (blob, cell index) pairs; every prefix of two or more repeats a commitment and holds the indices 0 and 127"""
    rng = random.Random("leaf-kernel:1")
    return [(0, 0), (0, 127), (1, 0), (2, 127)] + [(rng.choice((0, 1, 2, T.B_CONST)), rng.randrange(T.N_CELLS)) for _ in range(125)]


@pytest.mark.parametrize("n", LEAF_SIZES)
def test_leaf_kernel_digests_equal_hashlib(forms, material, n):
    lib = kzg.load_library()
    comm, idx, cells, proofs = T.CellCase("leaves-%d" % n, _leaf_entries()[:n]).args(material)
    assert len(idx) == n and idx[0] == 0 and (n == 1 or (127 in idx and len(set(comm)) < n))
    want = b"".join(L.leaf_digests(comm, idx, cells, proofs))
    ia = np.array(idx, dtype=np.uint64)
    for form, ctx in forms.items():
        out = C.create_string_buffer(32 * n)
        rc = lib.eth_kzg_amd_test_cell_leaf_digests(ctx.handle, n, b"".join(comm), kzg._vp(ia), b"".join(cells), b"".join(proofs), out)
        assert rc == 0, (form, n, rc)
        bad = [k for k in range(n) if out.raw[32 * k:32 * k + 32] != want[32 * k:32 * k + 32]]
        assert not bad, (form, n, bad)


def test_leaf_hook_refuses_what_validation_refuses(forms):
    lib = kzg.load_library()
    ctx = forms["windowed"]
    out = C.create_string_buffer(32)
    one = np.array([128], dtype=np.uint64)
    assert lib.eth_kzg_amd_test_cell_leaf_digests(ctx.handle, 1, bytes(48), kzg._vp(one), bytes(2048), bytes(48), out) == 3
    assert lib.eth_kzg_amd_test_cell_leaf_digests(ctx.handle, 0, bytes(48), kzg._vp(one), bytes(2048), bytes(48), out) == 3
    assert lib.eth_kzg_amd_test_cell_leaf_digests(None, 1, None, None, None, None, out) == 3
    assert lib.eth_kzg_amd_test_verify_cells_inputs_ex(None, 1, 0, None, None, None, None, LEAF, out, out) == 3


# ---- 2. the root and the pairing inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INPUT_CASES)
def test_root_and_pairing_inputs_equal_the_statement(forms, material, name):
    case = CASES[name]
    case.check(material)
    args = case.args(material)
    n = len(args[1])
    assert n <= 300
    device_arrays = _device_arrays(args) if name in DEVICE_CASES else None
    bad = []
    for flags in (LEAF, 0):
        want_root, want96 = _want(material, case, flags)
        for form, ctx in forms.items():
            for where, arrays in [("host", None)] + ([("device", device_arrays)] if device_arrays else []):
                rc, root, out96 = _inputs_ex(ctx, args, flags, arrays)
                assert rc == 0, (name, flags, form, where, rc)
                if root != want_root or out96 != want96:
                    bad.append((flags, form, where, root == want_root, out96[:48] == want96[:48], out96[48:] == want96[48:]))
    assert not bad, "%s: (flags, form, where, root equal, A equal, B equal) %s" % (name, bad)
    assert _want(material, case, LEAF)[0] != _want(material, case, 0)[0]
    for form, ctx in forms.items():
        assert ctx.verify_cell_kzg_proof_batch(*args, leaf_transcript=True) is True, (name, form)
        if device_arrays:
            d_c, d_i, d_l, d_p = device_arrays
            assert ctx.verify_cell_kzg_proof_batch_device(n, d_c.data_ptr(), d_i.data_ptr(), d_l.data_ptr(), d_p.data_ptr(), leaf_transcript=True) is True


# ---- 3. errors and wrong proofs --------------------------------------------------------------------------------------------------------
def _outcome(fn, *a, **kw):
    """-> ("ok", verdict) or ("err", the message up to its first colon)"""
    try:
        return "ok", fn(*a, **kw)
    except kzg.KzgError as e:
        return "err", str(e).split(":")[0]


@pytest.mark.parametrize("kind", ["swapped", "bad-index", "bad-scalar", "off-subgroup"])
def test_flagged_and_unflagged_calls_agree_on_errors_and_wrong_proofs(forms, material, kind):
    case = CASES["len-65"]
    proofs = case.args(material)[3]
    swap = next((i, j) for i in range(65) for j in range(i + 1, 65) if proofs[i] != proofs[j])
    args = T.ManyProblem(case, kind, swap=swap).args(material)
    n = len(args[1])
    d_c, d_i, d_l, d_p = _device_arrays(args)
    ptrs = (n, d_c.data_ptr(), d_i.data_ptr(), d_l.data_ptr(), d_p.data_ptr())
    for form, ctx in forms.items():
        want = _outcome(ctx.verify_cell_kzg_proof_batch, *args)
        if kind == "swapped":
            assert want == ("ok", False), form
        else:
            assert want[0] == "err", (form, want)
        assert _outcome(ctx.verify_cell_kzg_proof_batch, *args, leaf_transcript=True) == want, (kind, form, "host")
        assert _outcome(ctx.verify_cell_kzg_proof_batch_device, *ptrs) == want, (kind, form, "device, unflagged")
        assert _outcome(ctx.verify_cell_kzg_proof_batch_device, *ptrs, leaf_transcript=True) == want, (kind, form, "device")


def test_empty_batches_verify_and_unknown_flags_are_invalid_input(forms):
    lib = kzg.load_library()
    ctx = forms["shifted"]
    assert ctx.verify_cell_kzg_proof_batch([], [], [], [], leaf_transcript=True) is True
    assert ctx.verify_cell_kzg_proof_batch_device(0, 0, 0, 0, 0, leaf_transcript=True) is True
    ok = C.c_bool(False)
    for flags in (2, 3, 1 << 31):
        for handle in (None, ctx.handle):  # refused before the context is touched: a NULL context is never reached
            for res in (lib.eth_kzg_amd_verify_cell_kzg_proof_batch_ex(handle, 0, None, 0, None, 0, None, 0, None, flags, C.byref(ok)),
                        lib.eth_kzg_amd_verify_cell_kzg_proof_batch_device_ex(handle, 0, None, None, None, None, flags, C.byref(ok), None)):
                assert res.status == 1 and res.error_msg
                msg = C.string_at(res.error_msg).decode()
                lib.eth_kzg_free_error_message(res.error_msg)
                assert msg.startswith("InvalidInput"), msg
    # flags = 0 is the existing call
    res = lib.eth_kzg_amd_verify_cell_kzg_proof_batch_ex(ctx.handle, 0, None, 0, None, 0, None, 0, None, 0, C.byref(ok))
    assert res.status == 0 and ok.value is True
    assert lib.eth_kzg_amd_abi_version() == 6


# ---- 4. the reference's verdicts -------------------------------------------------------------------------------------------------------
GOLDEN = sorted(vectors.load("verify_cell_kzg_proof_batch").items())


def test_there_are_thirty_reference_cases():
    assert len(GOLDEN) == 30


@pytest.mark.parametrize("name,case", GOLDEN)
def test_flagged_call_gives_the_reference_verdicts(forms, name, case):
    i = case["input"]
    for form, ctx in forms.items():
        kind, got = _outcome(ctx.verify_cell_kzg_proof_batch, i["commitments"], i["cell_indices"], i["cells"], i["proofs"], leaf_transcript=True)
        assert (got if kind == "ok" else None) == case["output"], (name, form, kind, got)
