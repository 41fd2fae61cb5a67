"""Planned inputs for the G1 / G2 subgroup tests: points of small order, sums of a subgroup point and a small-order point, decoded y
right at the two ends of the "lexicographically largest" comparison, and the edges of the 48-byte encoding.  Pure Python integers,
deterministic (SHA-512 of fixed tags), every list built once per process.

A hash-made curve point has a full-order component in every prime of the cofactor, so Scott's test [z^2]P - P == phi(P) sees a
generic [z^2]P - P for it.  For a point S of order l | h the ladder instead meets acc == p, acc == -p and acc == O, and
[z^2]S - S is the identity itself, because z = 1 mod l for every prime l of h = (z - 1)^2 / 3.

The group law is device_ops' (G1) and setup_material's (G2); only multiplication by an integer that is NOT reduced mod r is added.
tests/test_small_order.py proves every claim made here in exact integers; the GPU tests take their expectations from g1_cases()."""
import functools
import hashlib
from collections import namedtuple

import device_ops as d
import setup_material as sm

P, R = d.P, d.R_ORDER
Z = -0xd201000000010000
H1 = (Z - 1) ** 2 // 3  # cofactor of E(Fp)
N1 = H1 * R  # #E(Fp)
G1_PRIMES = (3, 11, 10177, 859267, 52437899)
HALF = (P - 1) // 2
# #E'(Fp2) = H2 * r (the sextic twist that carries G2); re-derived from p and the trace in tests/test_small_order.py
H2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5
G2_PRIMES = (13, 23, 2713)
K_CONTROL = (1, 2, 0x1234567, R - 1, 0x3b9aca07d8f1e2c3a4b5968778695a4b3c2d1e0ff0e1d2c3b4a5968778695a4b)
K_MIXED = (5, 0x2f6b1d0c9e8a7b6c5d4e3f2a1b0c9d8e7f6a5b4c3d2e1f0a9b8c7d6e5f4a3b2c)
BOUNDARY_K = (4, 7, 8, 14, 15, 19)  # 15 and 19: a^((p+1)/4) is the LARGER root there, for the others the smaller (sqrt_is_large)
BOUNDARY_Y = (2, 7, 8)


# ---- exact arithmetic -----------------------------------------------------------------------------------------------------------
def g1_mul(a, k):
    """[k]a for any integer k (device_ops.g_mul reduces k mod r, which kills exactly what is of interest here)."""
    if k < 0:
        return g1_mul(d.g_neg(a), -k)
    r = None
    for bit in bin(k)[2:] if k else "":
        r = d.g_add(r, r)
        if bit == "1":
            r = d.g_add(r, a)
    return r


def g1_order(a, primes=G1_PRIMES):
    """The exact order of a point whose order divides h (None for a point h does not kill)."""
    if g1_mul(a, H1) is not None:
        return None
    n = H1
    for l in primes:
        while n % l == 0 and g1_mul(a, n // l) is None:
            n //= l
    return n


def g2_order(q):
    """The exact order of a point whose order divides 13^2 23^2 2713 (None for any other point)."""
    n = 13 * 13 * 23 * 23 * 2713
    if sm.g2_mul(q, n) is not None:
        return None
    for l in G2_PRIMES:
        while n % l == 0 and sm.g2_mul(q, n // l) is None:
            n //= l
    return n


def fp_sqrt(a):
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def fp_cbrts(a):
    """Every cube root of a in Fp.  p - 1 = 9 m with 3 not dividing m: a^(1/3 mod m) is a cube root up to an element of the 3-Sylow
    subgroup (9 elements), which is fixed by trying them."""
    a %= P
    if a == 0:
        return [0]
    m = (P - 1) // 9
    assert (P - 1) % 9 == 0 and m % 3 != 0
    c = pow(a, pow(3, -1, m), P)
    z9 = next(pow(g, m, P) for g in range(2, 50) if pow(g, (P - 1) // 3, P) != 1)
    assert pow(z9, 9, P) == 1 and pow(z9, 3, P) != 1
    return sorted({c * pow(z9, i, P) % P for i in range(9) if pow(c * pow(z9, i, P), 3, P) == a})


def sqrt_is_large(x):
    """Whether (x^3 + 4)^((p+1)/4), the root every decoder here computes first, is the lexicographically larger one: a decoder's sign
    predicate is wrong VISIBLY only where its answer for that root differs from the exact rule's."""
    return fp_sqrt(x ** 3 + 4) > HALF


def hashed_g1(tag):
    """A curve point from SHA-512 of a tag: the first x >= the digest mod p with a square right-hand side, the smaller y."""
    x = int.from_bytes(hashlib.sha512(b"small_order/g1/" + tag).digest(), "big") % P
    while True:
        y = fp_sqrt(x ** 3 + 4)
        if y is not None:
            return x, min(y, P - y)
        x = (x + 1) % P


def g2_seed_point(start):
    """The first x = c + u, c >= start, that is the abscissa of a point of E'(Fp2)."""
    for c in range(start, start + 200):
        x = (c, 1)
        y = sm.f2_sqrt(sm.f2_add(sm.f2_mul(sm.f2_sqr(x), x), sm.B2))
        if y is not None:
            return x, y
    raise AssertionError("no curve point found")


def psi(q):
    """The untwist-Frobenius-twist endomorphism of E'(Fp2): (x, y) -> (conj(x) / xi^((p-1)/3), conj(y) / xi^((p-1)/2)), xi = 1 + u."""
    if q is None:
        return None
    cx = sm.f2_inv(sm.f2_pow((1, 1), (P - 1) // 3))
    cy = sm.f2_inv(sm.f2_pow((1, 1), (P - 1) // 2))
    (x0, x1), (y0, y1) = q
    return sm.f2_mul((x0, -x1 % P), cx), sm.f2_mul((y0, -y1 % P), cy)


# ---- the exact rule for a 48-byte encoding -----------------------------------------------------------------------------------------
def encode(a, flip=False):
    b = bytearray(d.compress(a))
    if flip:
        b[0] ^= 0x20
    return bytes(b)


def decode(enc):
    """-> (status, point): 0 and the affine point (None = identity), or 1 (bad encoding, x >= p, not on the curve) and None."""
    b0 = enc[0]
    x = int.from_bytes(enc, "big") & ((1 << 381) - 1)
    if not b0 & 0x80:
        return 1, None
    if b0 & 0x40:
        return (1, None) if (b0 & 0x20 or x) else (0, None)
    if x >= P:
        return 1, None
    y = fp_sqrt(x ** 3 + 4)
    if y is None:
        return 1, None
    if (y > HALF) != bool(b0 & 0x20):
        y = P - y
    return 0, (x, y)


Case = namedtuple("Case", "name enc status0 status1 xy0 xy1 point")
# status0 / xy0: decoding without the subgroup test; status1 / xy1: with it.  xy = 96 bytes, x | y big-endian, zero for the
# identity and for a refused point.  point: the decoded affine point (None: identity or undecodable).


def xy_bytes(a):
    return bytes(96) if a is None else a[0].to_bytes(48, "big") + a[1].to_bytes(48, "big")


def make_case(name, enc):
    st, pt = decode(enc)
    if st:
        return Case(name, enc, 1, 1, bytes(96), bytes(96), None)
    in_subgroup = g1_mul(pt, R) is None
    return Case(name, enc, 0, 0 if in_subgroup else 2, xy_bytes(pt), xy_bytes(pt) if in_subgroup else bytes(96), pt)


# ---- G1 lists -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_order_points():
    """{l: S_l}, S_l of order exactly l, for the five primes of the cofactor."""
    out = {}
    for l in G1_PRIMES:
        e = 0
        while N1 % l ** (e + 1) == 0:
            e += 1
        for attempt in range(8):
            s = g1_mul(hashed_g1(b"seed %d %d" % (l, attempt)), N1 // l ** e)
            if s is not None:
                break
        else:
            raise AssertionError("no point of order %d" % l)
        while True:
            t = g1_mul(s, l)
            if t is None:
                break
            s = t
        out[l] = s
    return out


@functools.lru_cache(maxsize=None)
def control_points():
    return tuple(d.g_mul(d.G, k) for k in K_CONTROL)


@functools.lru_cache(maxsize=None)
def boundary_points():
    """[(label, point)]: y = (p-1)/2 - k and (p+1)/2 + k for k in BOUNDARY_K (decided in the LOWEST word of the comparison with (p-1)/2)
    and y = 2, 7, 8, p - 2, p - 7, p - 8 (the eleven high words all zero, or all equal to p's)."""
    out = []
    for k in BOUNDARY_K:
        for label, y in (("half-%d" % k, HALF - k), ("half+1+%d" % k, HALF + 1 + k)):
            out.append((label, (fp_cbrts(y * y - 4)[0], y)))
    for k in BOUNDARY_Y:
        for label, y in (("y=%d" % k, k), ("y=p-%d" % k, P - k)):
            out.append((label, (fp_cbrts(y * y - 4)[0], y)))
    return tuple(out)


def _raw(flags, x):
    b = bytearray(x.to_bytes(48, "big"))
    assert b[0] < 0x20
    b[0] |= flags
    return bytes(b)


@functools.lru_cache(maxsize=None)
def g1_cases():
    """Every planned 48-byte encoding with what the exact rule says about it, in a fixed order."""
    S = small_order_points()
    cases = []
    for l in G1_PRIMES:
        cases.append(make_case("S_%d" % l, encode(S[l])))
        cases.append(make_case("-S_%d" % l, encode(d.g_neg(S[l]))))
    cases.append(make_case("S_3+S_11", encode(d.g_add(S[3], S[11]))))
    cases.append(make_case("S_11+S_10177", encode(d.g_add(S[11], S[10177]))))
    for k in K_MIXED:
        q = d.g_mul(d.G, k)
        for l in G1_PRIMES:
            cases.append(make_case("[%x]G+S_%d" % (k & 0xffff, l), encode(d.g_add(q, S[l]))))
    cases.append(make_case("identity", encode(None)))
    for k, q in zip(K_CONTROL, control_points()):
        cases.append(make_case("[%x]G" % (k & 0xffff), encode(q)))
    for label, pt in boundary_points():
        cases.append(make_case(label, encode(pt)))
        cases.append(make_case(label + " flipped", encode(pt, flip=True)))
    for label, x in (("x=p-1", P - 1), ("x=p", P), ("x=p+1", P + 1), ("x=2^381-1", (1 << 381) - 1)):
        for flags in (0x80, 0xa0, 0x00, 0x20):
            cases.append(make_case("%s flags %02x" % (label, flags), _raw(flags, x)))
    for x in (0, 1):
        for top in range(8):
            cases.append(make_case("x=%d top bits %d" % (x, top), _raw(top << 5, x)))
    cases.append(make_case("infinity with sign", _raw(0xe0, 0)))
    cases.append(make_case("infinity, x non-zero in the last byte", _raw(0xc0, 1)))
    cases.append(make_case("infinity, x non-zero in the first word", _raw(0xc0, 1 << 352)))
    return tuple(cases)


N_G1_CASES = 10 + 2 + 10 + 1 + 5 + 36 + 16 + 16 + 3


def planted(l, mixed):
    """The encoding the public-route tests plant: S_l, or [k]G + S_l."""
    name = ("[%x]G+S_%d" % (K_MIXED[1] & 0xffff, l)) if mixed else "S_%d" % l
    return next(c for c in g1_cases() if c.name == name)


def off_subgroup_cases():
    """The 22 planned points a subgroup test alone can refuse: every +-S_l, the two composite-order points, every [k]G + S_l."""
    out = [c for c in g1_cases() if c.name.lstrip("-").startswith("S_") or "+S_" in c.name]
    assert len(out) == 22 and all((c.status0, c.status1) == (0, 2) for c in out)
    return out


MANY_PLANTED = (0, 2, 4, 6, 8, 10)
MANY_STATUS = [2 if b in MANY_PLANTED else 0 for b in range(12)]
MANY_VERDICTS = [b in (1, 3, 5, 11) for b in range(12)]  # 3: the all-identity problem; 7 and 9 are well-formed and wrong


def many_plan(valid):
    """One many-verification call that hands the subgroup blocks of its pass EVERY off-subgroup case, the identity and valid controls.
    valid: 12 valid problems (commitments, indices, cells, proofs) of 8 cells each.  -> (base, planted): two lists of 12 problems.
    base: 3 = the zero polynomial's cells with the identity as commitment and as every proof (valid: True); 7 = the identity in the
    place of one proof (well-formed, False); 9 = a proof of problem 8 (well-formed, False); the rest as given.  planted: the same,
    but problem j of MANY_PLANTED carries chunk j of off_subgroup_cases() as proofs 0 .. and chunk j + 3 as commitments 4 .., so that
    every case appears once as a proof and once as a commitment: status MANY_STATUS, verdicts MANY_VERDICTS (a refused problem: False)."""
    assert len(valid) == 12 and all(len(p[1]) == 8 for p in valid)
    inf = encode(None)
    base = [tuple(list(x) for x in p) for p in valid]
    base[3] = ([inf] * 8, list(valid[3][1]), [bytes(2048)] * 8, [inf] * 8)
    base[7][3][2] = inf
    base[9][3][0] = valid[8][3][0]
    off = off_subgroup_cases()
    chunks = [off[4 * j:4 * j + 4] for j in range(6)]
    assert sum(len(c) for c in chunks) == 22 and all(chunks)
    planted = [tuple(list(x) for x in p) for p in base]
    for j, b in enumerate(MANY_PLANTED):
        for i, c in enumerate(chunks[j]):
            planted[b][3][i] = c.enc
        for i, c in enumerate(chunks[(j + 3) % 6]):
            planted[b][0][4 + i] = c.enc
    assert sorted(e for b in MANY_PLANTED for e in planted[b][3][:4] if e not in valid[b][3]) == sorted(c.enc for c in off)
    assert sorted(e for b in MANY_PLANTED for e in planted[b][0][4:] if e not in valid[b][0]) == sorted(c.enc for c in off)
    return base, planted


# ---- G2 lists -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g2_small_order_points():
    """{l: S_l} of order exactly l in E'(Fp2), l = 13, 23, 2713, from x = c + u curve points."""
    n2 = H2 * R
    out = {}
    for l in G2_PRIMES:
        e = 0
        while n2 % l ** (e + 1) == 0:
            e += 1
        c = 1
        while True:
            seed = g2_seed_point(c)
            s = sm.g2_mul(seed, n2 // l ** e)
            if s is not None:
                break
            c = seed[0][0] + 1
        while True:
            t = sm.g2_mul(s, l)
            if t is None:
                break
            s = t
        out[l] = s
    return out


@functools.lru_cache(maxsize=None)
def g2_points():
    """[(label, point)]: S_l, then [k][1]_2 + S_l."""
    S = g2_small_order_points()
    out = [("S_%d" % l, S[l]) for l in G2_PRIMES]
    q = sm.g2_mul(sm.G2_GEN, K_MIXED[0])
    out += [("[5][1]_2+S_%d" % l, sm.g2_add(q, S[l])) for l in G2_PRIMES]
    return tuple(out)


N_G2_POINTS = 6


def g2_decode(enc):
    """A valid 96-byte encoding of a finite point -> the affine point (the inverse of setup_material.g2_compress)."""
    assert len(enc) == 96 and enc[0] & 0xc0 == 0x80
    x = (int.from_bytes(enc[48:], "big"), int.from_bytes(enc[:48], "big") & ((1 << 381) - 1))
    y = sm.f2_sqrt(sm.f2_add(sm.f2_mul(sm.f2_sqr(x), x), sm.B2))
    assert y is not None
    q = (x, y)
    return q if sm.g2_compress(q) == enc else (x, sm.f2_sub((0, 0), y))


def g2_encodings():
    return b"".join(sm.g2_compress(q) for _, q in g2_points())
