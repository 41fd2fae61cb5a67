"""The planned points of tests/small_order.py, proved in exact integers (no GPU): the group orders and their factors are re-derived
here, every point is on its curve and has exactly the stated order, r kills none of the off-subgroup points, [z^2]S - S is the identity
for the pure small-order points (so Scott's test decides them in its is_inf branch), and psi(S) != [x]S on G2.  The CPU oracle's
validator must agree with the exact rule on every G1 encoding, in verdict and in the sign it decodes."""
import math

import pytest

import device_ops as d
import oracle_lib
import setup_material as sm
import small_order as so

P, R, Z = so.P, so.R, so.Z


def test_group_orders_and_their_factors():
    assert 3 * so.H1 == (Z - 1) ** 2
    assert so.H1 == 3 * 11 ** 2 * 10177 ** 2 * 859267 ** 2 * 52437899 ** 2
    assert all(Z % l == 1 for l in so.G1_PRIMES)  # why [z^2]S - S = O
    assert R == Z ** 4 - Z ** 2 + 1 and P == (Z - 1) ** 2 * R // 3 + Z
    t = P + 1 - so.H1 * R  # trace of Frobenius of E(Fp)
    assert abs(t) <= 2 * math.isqrt(P) + 1
    t2 = t * t - 2 * P  # trace over Fp2
    f = math.isqrt((4 * P * P - t2 * t2) // 3)
    assert 3 * f * f == 4 * P * P - t2 * t2
    n2 = P * P + 1 - (-3 * f + t2) // 2  # the sextic twist of order divisible by r
    assert (-3 * f + t2) % 2 == 0 and n2 == so.H2 * R
    small = 13 ** 2 * 23 ** 2 * 2713 * 11953 * 262069
    assert so.H2 % small == 0 and (so.H2 // small).bit_length() == 448
    assert all(math.gcd(so.H2 // small, l) == 1 for l in so.G2_PRIMES)
    # the seed points generate the whole group order: r [H] kills a hash-made point of either curve
    assert so.g1_mul(so.hashed_g1(b"order check"), so.N1) is None
    assert sm.g2_mul(so.g2_seed_point(1), n2) is None


def test_g1_small_order_points_have_exactly_the_stated_order():
    S = so.small_order_points()
    assert sorted(S) == list(so.G1_PRIMES)
    z2 = Z * Z
    for l, s in S.items():
        assert s is not None and d.on_curve(s)
        assert so.g1_mul(s, l) is None and so.g1_order(s) == l
        assert so.g1_mul(s, R) is not None
        for pt in (s, d.g_neg(s)):
            assert d.g_add(so.g1_mul(pt, z2), d.g_neg(pt)) is None  # [z^2]S - S = O: the verdict comes from the is_inf branch
    assert {S[3], d.g_neg(S[3])} == {(0, 2), (0, P - 2)}
    assert {so.encode((0, 2)), so.encode((0, P - 2))} == {b"\x80" + bytes(47), b"\xa0" + bytes(47)}
    assert so.g1_order(d.g_add(S[3], S[11])) == 33 and so.g1_order(d.g_add(S[11], S[10177])) == 11 * 10177
    beta = d.BETA
    for k in so.K_MIXED:
        q = d.g_mul(d.G, k)
        assert so.g1_mul(q, R) is None
        for l in so.G1_PRIMES:
            t = d.g_add(q, S[l])
            assert d.on_curve(t) and so.g1_mul(t, R) is not None
            lhs = d.g_add(so.g1_mul(t, z2), d.g_neg(t))
            assert lhs is not None
            assert all(lhs != (t[0] * b % P, t[1]) for b in (beta, beta * beta % P))  # Scott's relation is false for either cube root
    for q in so.control_points():
        assert q is not None and d.on_curve(q) and so.g1_mul(q, R) is None
        lhs = d.g_add(so.g1_mul(q, z2), d.g_neg(q))
        assert any(lhs == (q[0] * b % P, q[1]) for b in (beta, beta * beta % P))


def test_boundary_y_points():
    pts = dict(so.boundary_points())
    assert len(pts) == 18
    for k in so.BOUNDARY_K:
        lo, hi = pts["half-%d" % k], pts["half+1+%d" % k]
        assert lo[1] == so.HALF - k and hi[1] == so.HALF + 1 + k and lo[0] == hi[0] and (lo[1] + hi[1]) % P == 0
        # the comparison with (p-1)/2 is decided in the lowest 32-bit word: the eleven high words are equal
        assert lo[1] >> 32 == so.HALF >> 32 == hi[1] >> 32
    for k in so.BOUNDARY_Y:
        lo, hi = pts["y=%d" % k], pts["y=p-%d" % k]
        assert lo[1] == k and hi[1] == P - k and lo[0] == hi[0]
        assert hi[1] >> 32 == P >> 32
    for pt in pts.values():
        assert d.on_curve(pt)
        st, dec = so.decode(so.encode(pt))
        assert st == 0 and dec == pt
        st, dec = so.decode(so.encode(pt, flip=True))
        assert st == 0 and dec == d.g_neg(pt)
    # A wrong sign predicate shows only where its answer for the root the decoder computes first, a^((p+1)/4), is wrong: both kinds of
    # abscissa are present on either list (k = 4, 7, 8 alone give the smaller root three times, and a predicate that reads the top
    # word only decodes those correctly)
    assert {so.sqrt_is_large(pts["half-%d" % k][0]) for k in so.BOUNDARY_K} == {True, False}
    assert {so.sqrt_is_large(pts["y=%d" % k][0]) for k in so.BOUNDARY_Y} == {True, False}
    assert so.fp_cbrts(2) == [] or all(pow(c, 3, P) == 2 for c in so.fp_cbrts(2))
    assert len(so.fp_cbrts(8)) == 3 and 2 in so.fp_cbrts(8)


def test_g1_case_list_is_complete_and_the_oracle_agrees():
    cases = so.g1_cases()
    assert len(cases) == so.N_G1_CASES == 99
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    by = {c.name: c for c in cases}
    for l in so.G1_PRIMES:
        for name in ("S_%d" % l, "-S_%d" % l):
            assert (by[name].status0, by[name].status1) == (0, 2)
        assert (by["S_%d" % l].point[1] + by["-S_%d" % l].point[1]) % P == 0
    assert sum(c.name.startswith("[") and "+S_" in c.name for c in cases) == 10
    assert all((c.status0, c.status1) == (0, 2) for c in cases if "+S_" in c.name)
    assert (by["identity"].status0, by["identity"].status1, by["identity"].xy1) == (0, 0, bytes(96))
    controls = [c for c in cases if c.name.startswith("[") and "+S_" not in c.name]
    assert len(controls) == 5 and all(c.status1 == 0 and c.xy1 == so.xy_bytes(c.point) for c in controls)
    assert sum("flipped" in c.name for c in cases) == 18
    assert all(c.status1 == 2 for label, _ in so.boundary_points() for c in (by[label], by[label + " flipped"]))
    for c in cases:
        if "flipped" in c.name:
            plain = by[c.name[:-len(" flipped")]]
            assert c.status0 == 0 and c.point == d.g_neg(plain.point) and c.enc[1:] == plain.enc[1:] and c.enc[0] ^ plain.enc[0] == 0x20
    # the encoding edges: what the exact rule says about them
    assert by["x=p flags 80"].status0 == by["x=p+1 flags a0"].status0 == by["x=2^381-1 flags 80"].status0 == 1
    assert all(by["x=%d top bits %d" % (x, t)].status0 == 1 for x in (0, 1) for t in (0, 1, 2, 3, 7))
    assert by["x=0 top bits 4"].point == (0, 2) and by["x=0 top bits 5"].point == (0, P - 2)
    assert by["x=0 top bits 6"].status1 == 0 and by["x=1 top bits 6"].status0 == 1
    assert by["x=p-1 flags 80"].status0 == (0 if so.fp_sqrt(3) is not None else 1)
    assert by["x=1 top bits 4"].status0 == (0 if so.fp_sqrt(5) is not None else 1)
    assert all(by[n].status0 == 1 for n in names if n.startswith("infinity"))
    assert {c.status0 for c in cases} == {0, 1} and {c.status1 for c in cases} == {0, 1, 2}
    for c in cases:
        assert len(c.enc) == 48 and len(c.xy0) == len(c.xy1) == 96
        assert (oracle_lib.g1_validate(c.enc, False) == 0) == (c.status0 == 0), c.name
        assert (oracle_lib.g1_validate(c.enc, True) == 0) == (c.status1 == 0), c.name
        if c.point is not None:
            assert d.on_curve(c.point)
            assert oracle_lib.g1_validate(c.enc, False) == 0, c.name
            if c.status1 == 2:
                assert oracle_lib.g1_validate(c.enc, True) != 0, c.name
            # the oracle's decoded sign against the exact rule y > (p-1)/2: doubling through the oracle needs no subgroup
            # membership, and [2]P depends on the sign of y
            assert bool(c.enc[0] & 0x20) == (c.point[1] > so.HALF), c.name
            two = oracle_lib.g1_mul(c.enc, (2).to_bytes(32, "big"))
            assert two == d.compress(d.g_add(c.point, c.point)), c.name


def test_the_many_verification_plan_holds_every_off_subgroup_case_in_both_roles():
    off = so.off_subgroup_cases()
    assert len(off) == 22 and len({c.enc for c in off}) == 22
    assert sum(c.name.lstrip("-").startswith("S_") and "+" not in c.name for c in off) == 10 and sum("+S_" in c.name for c in off) == 12
    valid = [([b"C%047d" % b] * 8, list(range(8)), [bytes([b, i]) * 1024 for i in range(8)],
              [b"P%045d%02d" % (b, i) for i in range(8)]) for b in range(12)]
    base, planted = so.many_plan(valid)
    inf = so.encode(None)
    encs = {c.enc for c in off}
    assert len(base) == len(planted) == 12 and all(len(x) == 8 for p in base + planted for x in p)
    assert all(len(e) == 48 for p in planted for e in p[0] + p[3]) and all(len(cell) == 2048 for p in planted for cell in p[2])
    for b in range(12):
        bad = [e for e in planted[b][0] + planted[b][3] if e in encs]
        assert (len(bad) > 0) == (b in so.MANY_PLANTED) == (so.MANY_STATUS[b] == 2)
        if b not in so.MANY_PLANTED:
            assert planted[b] == base[b]
        assert planted[b][1] == base[b][1] and planted[b][2] == base[b][2]  # indices and cells stay
    assert {e for b in so.MANY_PLANTED for e in planted[b][3]} >= encs and {e for b in so.MANY_PLANTED for e in planted[b][0]} >= encs
    assert planted[3][0] == planted[3][3] == [inf] * 8 and planted[7][3].count(inf) == 1 and inf not in planted[7][0]
    assert not any(so.MANY_VERDICTS[b] for b in so.MANY_PLANTED) and so.MANY_VERDICTS[3] and not so.MANY_VERDICTS[7] and not so.MANY_VERDICTS[9]


@pytest.mark.timeout(600)
def test_g2_small_order_points():
    S = so.g2_small_order_points()
    assert sorted(S) == list(so.G2_PRIMES)
    x_abs = -Z
    for l, s in S.items():
        assert s is not None and sm.g2_on_curve(s)
        assert sm.g2_mul(s, l) is None and so.g2_order(s) == l
        assert sm.g2_mul(s, R) is not None
    pts = so.g2_points()
    assert len(pts) == so.N_G2_POINTS == 6 and len(so.g2_encodings()) == 6 * 96
    # psi is the endomorphism the host's test uses: on the subgroup it acts as multiplication by p, i.e. psi(Q) = [z]Q
    gen_z = sm.g2_mul(sm.G2_GEN, x_abs)
    assert so.psi(sm.G2_GEN) == (gen_z[0], sm.f2_sub((0, 0), gen_z[1]))
    for label, q in pts:
        assert sm.g2_on_curve(q) and sm.g2_mul(q, R) is not None, label
        zq = sm.g2_mul(q, x_abs)
        zq = None if zq is None else (zq[0], sm.f2_sub((0, 0), zq[1]))  # [z]Q, z < 0
        assert sm.g2_on_curve(so.psi(q)) and so.psi(q) != zq, label
