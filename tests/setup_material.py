"""Test material for caller-supplied trusted setups: an INSECURE setup with a known secret tau, generated (not committed), plus
the small pure-Python Fp2 / G2 arithmetic it needs -- the oracle exports G1 multiplication but nothing on G2.

    g1[i+1] = tau * g1[i]  by 4095 calls of oracle_g1_mul from the generator,
    g2[i]   = [tau^i]_2    by double-and-add on E'(Fp2): y^2 = x^3 + 4(1 + u), ZCash compression.

The known secret gives closed forms that depend on no KZG code: commitment = [p(tau)] G, proof_k = [(p(tau) - I_k(tau)) /
(tau^64 - h_k^64)] G (tests/test_gpu_custom_setup.py).  Generation is cached in a directory the caller names."""
import hashlib
import os

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAINNET_BIN = os.path.join(ROOT, "rust-eth-kzg_amd", "data", "trusted_setup_4096.bin")

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N_G1, N_G2 = 4096, 65
# fixed 255-bit secrets below r (digits of pi and e: nothing up the sleeve, and no security is claimed)
TAU = 0x7243f6a8885a308d313198a2e03707344a4093822299f31d0082efa98ec4e6c8
TAU_OTHER = 0x6b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe
assert TAU < R and TAU_OTHER < R and TAU.bit_length() == 255

G2_GEN = ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
           0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
          (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
           0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be))


# ---- Fp2 = Fp[u] / (u^2 + 1): pairs (c0, c1) ----
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_sqr(a):
    return f2_mul(a, a)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_sqr(a)
        e >>= 1
    return r


def f2_sqrt(a):
    """A square root in Fp2, or None (p = 3 mod 4: Adj & Rodriguez-Henriquez, algorithm 9)."""
    if a == (0, 0):
        return a
    a1 = f2_pow(a, (P - 3) // 4)
    x0 = f2_mul(a1, a)
    alpha = f2_mul(a1, x0)
    if alpha == (P - 1, 0):
        x = (-x0[1] % P, x0[0])
    else:
        x = f2_mul(f2_pow(f2_add(alpha, (1, 0)), (P - 1) // 2), x0)
    return x if f2_sqr(x) == a else None


B2 = (4, 4)


# ---- E'(Fp2) in affine coordinates; None is the point at infinity ----
def g2_on_curve(q):
    return q is None or f2_sqr(q[1]) == f2_add(f2_mul(f2_sqr(q[0]), q[0]), B2)


def g2_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if f2_add(a[1], b[1]) == (0, 0):
            return None
        lam = f2_mul(f2_mul((3, 0), f2_sqr(a[0])), f2_inv(f2_add(a[1], a[1])))
    else:
        lam = f2_mul(f2_sub(b[1], a[1]), f2_inv(f2_sub(b[0], a[0])))
    x = f2_sub(f2_sub(f2_sqr(lam), a[0]), b[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(a[0], x)), a[1]))


def g2_mul(q, k):
    r = None
    while k:
        if k & 1:
            r = g2_add(r, q)
        q = g2_add(q, q)
        k >>= 1
    return r


def g2_compress(q):
    """ZCash encoding: x.c1 | x.c0 big endian, flags in the top three bits (compressed, infinity, y lexicographically largest)."""
    if q is None:
        return bytes([0xc0]) + bytes(95)
    (x0, x1), (y0, y1) = q
    largest = y1 > (P - 1) // 2 if y1 else y0 > (P - 1) // 2
    b = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if largest else 0)
    return bytes(b)


def g2_off_subgroup_point():
    """A point of E'(Fp2) outside the order-r subgroup: the first x = c + u with a square right-hand side whose point r does not kill."""
    for c in range(1, 200):
        x = (c, 1)
        y = f2_sqrt(f2_add(f2_mul(f2_sqr(x), x), B2))
        if y is None:
            continue
        q = (x, y)
        assert g2_on_curve(q)
        if g2_mul(q, R) is not None:
            return q
    raise AssertionError("no curve point found")


def g1_off_subgroup_point():
    """48 bytes: a compressed point of E(Fp) outside the subgroup (the oracle's validator decides)."""
    for x in range(1, 500):
        b = bytearray(x.to_bytes(48, "big"))
        b[0] |= 0x80
        if oracle_lib.g1_validate(bytes(b), False) == 0 and oracle_lib.g1_validate(bytes(b), True) != 0:
            return bytes(b)
    raise AssertionError("no curve point found")


# ---- setups ----
def mainnet_points():
    raw = open(MAINNET_BIN, "rb").read()
    assert raw[:8] == b"KZGSRS01" and int.from_bytes(raw[8:12], "little") == N_G1 and int.from_bytes(raw[12:16], "little") == N_G2
    g1 = raw[16:16 + N_G1 * 48]
    g2 = raw[16 + N_G1 * 48:]
    assert len(g2) == N_G2 * 96
    return g1, g2


def flat_file(g1, g2):
    """The "KZGSRS01" layout the library embeds, the oracle parses and eth_kzg_amd_das_context_new_with_setup_file takes."""
    return b"KZGSRS01" + (len(g1) // 48).to_bytes(4, "little") + (len(g2) // 96).to_bytes(4, "little") + g1 + g2


def g1_powers(tau, n=N_G1):
    gen = mainnet_points()[0][:48]
    k = tau.to_bytes(32, "big")
    pts = [gen]
    for _ in range(n - 1):
        pts.append(oracle_lib.g1_mul(pts[-1], k))
    return b"".join(pts)


def g2_powers(tau, n=N_G2):
    out, t = [], 1
    for _ in range(n):
        out.append(g2_compress(g2_mul(G2_GEN, t)))
        t = t * tau % R
    return b"".join(out)


def insecure_setup(cache_dir, tau=TAU):
    """(g1_monomial, g2_monomial) bytes of the setup with secret tau; generated once per cache directory."""
    path = os.path.join(str(cache_dir), "insecure_setup_%s.bin" % hashlib.sha256(tau.to_bytes(32, "big")).hexdigest()[:16])
    if os.path.exists(path):
        raw = open(path, "rb").read()
        return raw[16:16 + N_G1 * 48], raw[16 + N_G1 * 48:]
    g1, g2 = g1_powers(tau), g2_powers(tau)
    tmp = path + ".%d.tmp" % os.getpid()
    with open(tmp, "wb") as f:
        f.write(flat_file(g1, g2))
    os.replace(tmp, path)
    return g1, g2


def digest(g1, g2):
    return hashlib.sha256(g1 + g2).digest()


class SetupOracle(oracle_lib.Oracle):
    """The CPU oracle on an arbitrary setup (oracle_ctx_new takes the flat file)."""

    def __init__(self, g1, g2, use_precomp=False, threads=1):
        import ctypes as C
        self.lib = oracle_lib._lib()
        srs = flat_file(g1, g2)
        self.ctx = C.c_void_p(self.lib.oracle_ctx_new(srs, len(srs), int(use_precomp), threads))
        assert self.ctx.value, "oracle_ctx_new failed"


# ---- closed forms on a known tau ----
def brp(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


OMEGA_4096 = pow(7, (R - 1) // 4096, R)
OMEGA_8192 = pow(7, (R - 1) // 8192, R)


def blob_evals(blob):
    return [int.from_bytes(blob[32 * i:32 * i + 32], "big") for i in range(4096)]


def eval_blob_at(blob, z):
    """p(z) for the polynomial whose evaluations over the bit-reversed 4096th roots of unity are the blob (barycentric formula)."""
    ev = blob_evals(blob)
    roots = [pow(OMEGA_4096, brp(i, 12), R) for i in range(4096)]
    assert z not in roots
    s = 0
    for e, w in zip(ev, roots):
        if e:
            s = (s + e * w % R * pow(z - w, R - 2, R)) % R
    return s * (pow(z, 4096, R) - 1) % R * pow(4096, R - 2, R) % R


def cell_interpolant_at(cell, k, z):
    """I_k(z): the degree-63 polynomial through cell k's 64 evaluations, over the coset h_k * <omega_64> in bit-reversed order."""
    ev = [int.from_bytes(cell[32 * i:32 * i + 32], "big") for i in range(64)]
    h = pow(OMEGA_8192, brp(k, 7), R)
    w64 = pow(OMEGA_8192, 128, R)
    xs = [h * pow(w64, brp(j, 6), R) % R for j in range(64)]
    # barycentric on a coset of the 64th roots: I(z) = (z^64 - h^64) / (64 h^64) * sum_j e_j x_j / (z - x_j)
    h64 = pow(h, 64, R)
    s = 0
    for e, x in zip(ev, xs):
        s = (s + e * x % R * pow(z - x, R - 2, R)) % R
    return s * (pow(z, 64, R) - h64) % R * pow(64 * h64 % R, R - 2, R) % R, h64
