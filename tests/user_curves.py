"""User-defined curves at field sizes no built-in curve has (TEST INFRASTRUCTURE).

tests/golden/user_curves.json holds the parameters (ours: two supersingular families whose order is known without point
counting, found by tests/golden/make_user_curves_fixture.py) and, per curve the default reference build can hold
(bitlen(p) <= 521), the UNMODIFIED reference's answers to the batches below.  The batches themselves are not stored: they are
rebuilt here from the parameters by a SHAKE-256 stream, and the fixture keeps a SHA-256 of each so that a drift would show.

Three references, in order of authority:
  (a) Python integers (this file): affine group law, textbook ECDSA with libecc's digest truncation, modular square roots;
  (b) the restatement oracle (oracles.Oracle on the parameter dict);
  (c) the recorded answers of the unmodified reference.
tests/test_user_curves_host.py shows that they agree; tests/test_gpu_user_curves.py compares the GPU library with them.
"""
import hashlib
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "user_curves.json")
PARAM_KEYS = ("p", "a", "b", "order", "gx", "gy", "q")
PY_ITEMS = 16          # Python scalar multiplication is slow at 544 bits: (a) answers at most this many items per batch
WIDTHS = (6, 7, 8, 10, 12, 14, 16, 17)   # the saturated-word widths of the library (32-bit words)
G29_SIZES = (192, 224, 255, 256, 320, 384, 448, 511, 512, 521)   # field sizes that also get a radix-2^29 unit


def load():
    """{name: curve dict}: the parameters as ints, 'name', 'family' ('A' / 'B'), 'h', 'hash', 'ref' (recorded answers or None)"""
    with open(FIXTURE) as f:
        fx = json.load(f)
    out = {}
    for c in fx["curves"]:
        cv = {k: int(c[k], 16) for k in PARAM_KEYS}
        cv.update(name=c["name"], family=c["family"], h=c["h"], hash=c["hash"], why=c["why"], ref=c.get("ref"),
                  sha256=c.get("sha256", {}))
        out[c["name"]] = cv
    return out


def params(cv):
    return {k: cv[k] for k in PARAM_KEYS}


def pbits(cv):
    return cv["p"].bit_length()


def clen(cv):
    return (cv["p"].bit_length() + 7) // 8


def qlen(cv):
    return (cv["q"].bit_length() + 7) // 8


def words(cv):
    return next(w for w in WIDTHS if 32 * w >= pbits(cv))


def path_of(cv):
    """the path a handle of this curve takes in the library, for the record"""
    return "g29 generic + saturated" if pbits(cv) in G29_SIZES else "saturated only"


class Stream:
    """a reproducible byte stream: SHAKE-256 of a label, read front to back"""

    def __init__(self, label):
        self.x = hashlib.shake_256(label.encode())
        self.buf, self.pos = b"", 0

    def bytes(self, n):
        if self.pos + n > len(self.buf):
            self.buf = self.x.digest(max(2 * len(self.buf), self.pos + n, 1 << 14))
        self.pos += n
        return self.buf[self.pos - n:self.pos]

    def below(self, n):
        """an integer in [0, n), from 16 spare bytes (bias below 2^-128)"""
        return int.from_bytes(self.bytes((n.bit_length() + 7) // 8 + 16), "big") % n

    def between(self, lo, hi):
        return lo + self.below(hi - lo)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) Python integers
# ---------------------------------------------------------------------------------------------------------------------------
def is_prime(n):
    """trial division, then Miller-Rabin to 24 fixed bases"""
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97)
    if n < 2:
        return False
    for s in small:
        if n % s == 0:
            return n == s
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in small[:24]:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def on_curve(P, cv):
    p = cv["p"]
    return P is not None and 0 <= P[0] < p and 0 <= P[1] < p and (P[1] * P[1] - (P[0] ** 3 + cv["a"] * P[0] + cv["b"])) % p == 0


def add(P, Q, cv):
    """the affine group law; None is the point at infinity"""
    p = cv["p"]
    if P is None:
        return Q
    if Q is None:
        return P
    if P[0] == Q[0]:
        if (P[1] + Q[1]) % p == 0:
            return None
        lam = (3 * P[0] * P[0] + cv["a"]) * pow(2 * P[1], -1, p) % p
    else:
        lam = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
    x = (lam * lam - P[0] - Q[0]) % p
    return (x, (lam * (P[0] - x) - P[1]) % p)


def neg(P, cv):
    return None if P is None else (P[0], (-P[1]) % cv["p"])


def mul(k, P, cv):
    R = None
    while k:
        if k & 1:
            R = add(R, P, cv)
        P = add(P, P, cv)
        k >>= 1
    return R


def sqrt_mod(w, p):
    """a square root of w mod p, or None: the exponentiation for p = 3 (mod 4), Tonelli-Shanks otherwise"""
    w %= p
    if w == 0:
        return 0
    if pow(w, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(w, (p + 1) // 4, p)
    s, t = 0, p - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    c, x, b, m = pow(z, t, p), pow(w, (t + 1) // 2, p), pow(w, t, p), s
    while b != 1:
        i, b2 = 0, b
        while b2 != 1:
            b2, i = b2 * b2 % p, i + 1
        g = pow(c, 1 << (m - i - 1), p)
        x, c, b, m = x * g % p, g * g % p, b * g * g % p, i
    return x


def lift_x(x, cv):
    """a point with this abscissa, or None"""
    y = sqrt_mod(x ** 3 + cv["a"] * x + cv["b"], cv["p"])
    return None if y is None else (x, y)


def pt_bytes(P, cv):
    n = clen(cv)
    return bytes(2 * n) if P is None else P[0].to_bytes(n, "big") + P[1].to_bytes(n, "big")


def pt_from(buf, cv):
    """(x, y) as the bytes say, reduced or not"""
    n = clen(cv)
    return (int.from_bytes(buf[:n], "big"), int.from_bytes(buf[n:2 * n], "big"))


def digest_to_e(h, cv):
    """libecc's truncation: e = OS2I(h) >> max(0, 8 |h| - |q|) mod q, on the leftmost min(|h|, qlen) octets"""
    q = cv["q"]
    qb = q.bit_length()
    h = h[:min(len(h), qlen(cv))]
    e = int.from_bytes(h, "big")
    if 8 * len(h) > qb:
        e >>= 8 * len(h) - qb
    return e % q


def py_smul(cv, items):
    """prj_pt_mul + prj_pt_unique as the reference answers: status 0 and X || Y, 1 for a point that does not import or has order
    two (every step of the reference's ladder is then an exceptional pair of its complete addition), 2 for infinity"""
    out, st = [], []
    for k, B in items:
        P = (cv["gx"], cv["gy"]) if B is None else pt_from(B, cv)
        if not on_curve(P, cv) or P[1] == 0:
            out.append(pt_bytes(None, cv)), st.append(1)
            continue
        R = mul(k, P, cv)
        out.append(pt_bytes(R, cv)), st.append(2 if R is None else 0)
    return b"".join(out), bytes(st)


def py_add(cv, pairs, dbl=False):
    """prj_pt_add / prj_pt_dbl: status 1 also for the addition's exceptional pairs, P - Q of order exactly two"""
    out, st = [], []
    for A, B in pairs:
        P, Q = pt_from(A, cv), pt_from(A if dbl else B, cv)
        if not on_curve(P, cv) or not on_curve(Q, cv):
            out.append(pt_bytes(None, cv)), st.append(1)
            continue
        D = add(P, neg(Q, cv), cv)
        if not dbl and D is not None and D[1] == 0:
            out.append(pt_bytes(None, cv)), st.append(1)
            continue
        R = add(P, Q, cv)
        out.append(pt_bytes(R, cv)), st.append(2 if R is None else 0)
    return b"".join(out), bytes(st)


def py_sign(cv, items):
    """textbook ECDSA with the nonce supplied: (r || s, status) per (x, k, digest)"""
    q, n = cv["q"], qlen(cv)
    out, st = [], []
    for x, k, h in items:
        bad = not (0 < x < q and 0 < k < q)
        r = s = 0
        if not bad:
            r = mul(k, (cv["gx"], cv["gy"]), cv)[0] % q
            s = pow(k, -1, q) * (digest_to_e(h, cv) + x * r) % q
            bad = r == 0 or s == 0
        out.append(bytes(2 * n) if bad else r.to_bytes(n, "big") + s.to_bytes(n, "big")), st.append(1 if bad else 0)
    return b"".join(out), bytes(st)


def py_verify(cv, items):
    """0 accept / 1 reject per (public key bytes, r || s, digest); keys outside the generator's subgroup are rejected"""
    q, n = cv["q"], qlen(cv)
    G = (cv["gx"], cv["gy"])
    res = []
    for Y, sig, h in items:
        P = pt_from(Y, cv)
        r, s = int.from_bytes(sig[:n], "big"), int.from_bytes(sig[n:], "big")
        ok = on_curve(P, cv) and P[1] != 0 and mul(q, P, cv) is None and 0 < r < q and 0 < s < q
        if ok:
            w = pow(s, -1, q)
            W = add(mul(digest_to_e(h, cv) * w % q, G, cv), mul(r * w % q, P, cv), cv)
            ok = W is not None and W[0] % q == r
        res.append(0 if ok else 1)
    return bytes(res)


def py_y_from_x(cv, xs):
    """status 0 and the two roots as a set, or status 1 (x >= p, or no root)"""
    p, n = cv["p"], clen(cv)
    out = []
    for i in range(len(xs) // n):
        x = int.from_bytes(xs[n * i:n * (i + 1)], "big")
        y = sqrt_mod(x ** 3 + cv["a"] * x + cv["b"], p) if x < p else None
        out.append(None if y is None else {y, (p - y) % p})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the points of a curve the batches are made of
# ---------------------------------------------------------------------------------------------------------------------------
def special_points(cv):
    """{'sub': 4 points of the order-q subgroup, 'full': a point outside it with q dividing its order, 'two': a point of order
    two, 'low': the other points of small order that exist (order 4 on family A when the group is cyclic; 3 and 6 on B)}"""
    if "_pts" in cv:
        return cv["_pts"]
    p, q, h = cv["p"], cv["q"], cv["h"]
    rs = Stream("points/" + cv["name"])
    G = (cv["gx"], cv["gy"])
    sub = [mul(rs.between(2, q), G, cv) for _ in range(4)]
    full = None
    while full is None:
        R = lift_x(rs.below(p), cv)
        if R is not None and mul(q, R, cv) is not None and mul(h, R, cv) is not None:
            full = R
    if cv["family"] == "A":
        two = (0, 0)
    else:
        two = (pow((-cv["b"]) % p, (2 * p - 1) // 3, p), 0)     # the cube root is unique for p = 2 (mod 3)
    assert on_curve(two, cv)
    # points of small order: [q]R has an order dividing h.  Family A has points of order 4 iff (0, 0) is its only point of order
    # two (-a no square: the group is cyclic); family B is always cyclic (one cube root, and no full 3-torsion for p = 2 mod 3)
    low = {}
    if cv["family"] == "B" or pow((-cv["a"]) % p, (p - 1) // 2, p) != 1:
        while h not in low:
            R = lift_x(rs.below(p), cv)
            L = None if R is None else mul(q, R, cv)
            if L is not None and all(mul(e, L, cv) is not None for e in range(1, h)):
                low[h] = L
        if h == 6:
            low[3] = add(low[6], low[6], cv)
    cv["_pts"] = {"sub": sub, "full": full, "two": two, "low": low}
    return cv["_pts"]


def _sc(k, n):
    return k.to_bytes(n, "big")


def crafted_scalars(cv, slen):
    q, order = cv["q"], cv["order"]
    top = 1 << (8 * slen)
    vals = [0, 1, 2, q - 1, q, q + 1, order - 1, order, order + 1, 2 * q, top - 1, top >> 1]
    return [v for v in vals if v < top]


# ---------------------------------------------------------------------------------------------------------------------------
# the batches (every reference and the GPU library answer the same bytes)
# ---------------------------------------------------------------------------------------------------------------------------
def smul_batches(cv):
    """[(label, slen, scalars bytes, points bytes or None)]: fixed and variable base, scalars of qlen, qlen + 8 and qlen - 8 octets"""
    if "_smul" in cv:
        return cv["_smul"]
    p, q, ql, cl = cv["p"], cv["q"], qlen(cv), clen(cv)
    rs = Stream("smul/" + cv["name"])
    S = special_points(cv)
    out = []
    for tag, slen, nrand in (("q", ql, 16), ("long", ql + 8, 6), ("short", ql - 8, 6)):
        sc = crafted_scalars(cv, slen) + [rs.below(1 << (8 * slen)) for _ in range(nrand)]
        out.append(("fixed/" + tag, slen, b"".join(_sc(k, slen) for k in sc), None))
    bases = [pt_bytes(P, cv) for P in S["sub"][:2]] + [pt_bytes(S["full"], cv), pt_bytes(S["two"], cv)]
    bases += [pt_bytes(S["low"][d], cv) for d in sorted(S["low"])]
    # rejections: x = p, x + p with the same residue where it fits, off-curve, all-ones, y >= p
    P0 = S["sub"][0]
    bad = [_sc(p, cl) + _sc(P0[1], cl), _sc(P0[0], cl) + _sc((P0[1] + 1) % p, cl), b"\xff" * (2 * cl), bytes(2 * cl) if cv["b"] else
           _sc(0, cl) + _sc(1, cl)]
    if P0[0] + p < 1 << (8 * cl):
        bad.append(_sc(P0[0] + p, cl) + _sc(P0[1], cl))
    if P0[1] + p < 1 << (8 * cl):
        bad.append(_sc(P0[0], cl) + _sc(P0[1] + p, cl))
    top = 1 << (8 * ql)
    per_base = [0, 1, 2, 3, q, q + 1, cv["order"] - 1 if cv["order"] - 1 < top else q - 1, top - 1]
    sc, pts = [], []
    for B in bases + bad:
        for k in per_base + [rs.below(top) | 1, rs.below(top) & ~1, rs.below(top)]:
            sc.append(_sc(k, ql)), pts.append(B)
    out.append(("var/q", ql, b"".join(sc), b"".join(pts)))
    for tag, slen in (("long", ql + 8), ("short", ql - 8)):
        sc, pts = [], []
        for B in bases[:4]:
            for k in ([cv["order"], cv["order"] + 1] if tag == "long" else [1, 2]) + [rs.below(1 << (8 * slen)) for _ in range(2)]:
                sc.append(_sc(k, slen)), pts.append(B)
        out.append(("var/" + tag, slen, b"".join(sc), b"".join(pts)))
    cv["_smul"] = out
    return out


def add_batch(cv):
    """(P bytes, Q bytes, exc): the subgroup, P + P, P + (-P), points outside the subgroup; from index exc on the point of order
    two T as either operand and T + T, then the exceptional pairs Q = P + T (P - Q of order two), then operands that do not
    import"""
    if "_add" in cv:
        return cv["_add"]
    p, cl = cv["p"], clen(cv)
    rs = Stream("add/" + cv["name"])
    S = special_points(cv)
    G = (cv["gx"], cv["gy"])
    sub = S["sub"] + [mul(rs.between(2, cv["q"]), G, cv) for _ in range(4)]
    T = S["two"]
    pairs = [(sub[i], sub[(i + 1) % len(sub)]) for i in range(len(sub))]
    pairs += [(sub[0], sub[0]), (sub[1], neg(sub[1], cv)), (G, G), (G, neg(G, cv))]
    pairs += [(S["full"], sub[2]), (sub[3], S["full"]), (S["full"], S["full"]), (S["full"], neg(S["full"], cv))]
    pairs += [(S["low"][d], sub[0]) for d in sorted(S["low"])] + [(S["low"][d], S["low"][d]) for d in sorted(S["low"])]
    exc = len(pairs)
    pairs += [(T, sub[0]), (sub[1], T), (S["full"], T), (T, T)]
    pairs += [(P, add(P, T, cv)) for P in sub[:3]] + [(add(P, T, cv), P) for P in sub[3:5]]
    enc = [(pt_bytes(P, cv), pt_bytes(Q, cv)) for P, Q in pairs]
    good = pt_bytes(sub[0], cv)
    for B in (_sc(p, cl) + _sc(sub[0][1], cl), _sc(sub[0][0], cl) + _sc((sub[0][1] + 1) % p, cl), b"\xff" * (2 * cl)):
        enc += [(B, good), (good, B)]
    cv["_add"] = (b"".join(e[0] for e in enc), b"".join(e[1] for e in enc), exc)
    return cv["_add"]


def hash_of(cv):
    return {"SHA256": hashlib.sha256, "SHA512": hashlib.sha512}[cv["hash"]]


def sign_batch(cv):
    """(privs, nonces, msgs, msg_len, digests): random keys and nonces, the ends of [1, q - 1], and values the reference refuses"""
    if "_sign" in cv:
        return cv["_sign"]
    q, ql = cv["q"], qlen(cv)
    rs = Stream("sign/" + cv["name"])
    xs = [rs.between(1, q) for _ in range(12)] + [1, q - 1, rs.between(1, q), rs.between(1, q)]
    ks = [rs.between(1, q) for _ in range(12)] + [rs.between(1, q), rs.between(1, q), 1, q - 1]
    # (no private key 0: the reference refuses it where the key pair is imported, so its signer never sees one)
    xs += [q, q + 1, rs.between(1, q), rs.between(1, q)]
    ks += [rs.between(1, q), rs.between(1, q), 0, q]
    msgs = [rs.bytes(24) for _ in xs]
    cv["_sign"] = (b"".join(_sc(x, ql) for x in xs), b"".join(_sc(k, ql) for k in ks), b"".join(msgs), 24,
                   b"".join(hash_of(cv)(m).digest() for m in msgs))
    return cv["_sign"]


def _flip(buf, bit):
    b = bytearray(buf)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def verify_batch(cv):
    """(pubs, sigs, msgs, msg_len, digests, by_msg): valid signatures of this module's own signer, then one flipped bit in r, s,
    the message, the digest and the key, r or s equal to 0, q and q + 1, and keys outside the subgroup.  Item 9 flips a bit of the
    digest that e keeps, item 10 the digest's last bit: where the digest is longer than q that bit is shifted out and the signature
    stays valid.  by_msg[i] is False where
    the digest is not the hash of the message (a reference that hashes for itself cannot answer that item)."""
    if "_verify" in cv:
        return cv["_verify"]
    p, q, ql, cl = cv["p"], cv["q"], qlen(cv), clen(cv)
    rs = Stream("verify/" + cv["name"])
    S = special_points(cv)
    G = (cv["gx"], cv["gy"])
    H = hash_of(cv)
    base = []
    for _ in range(6):
        x, k, m = rs.between(1, q), rs.between(1, q), rs.bytes(24)
        sig, st = py_sign(cv, [(x, k, H(m).digest())])
        assert st == b"\x00"
        base.append((pt_bytes(mul(x, G, cv), cv), sig, m))
    items = [(Y, sig, m, None) for Y, sig, m in base]
    Y, sig, m = base[0]
    dg = H(m).digest()
    items += [(Y, _flip(sig, rs.below(8 * ql)), m, None), (Y, _flip(sig, 8 * ql + rs.below(8 * ql)), m, None),
              (Y, sig, _flip(m, rs.below(8 * len(m))), None), (Y, sig, m, _flip(dg, rs.below(8 * min(len(dg), q.bit_length() // 8)))),
              (Y, sig, m, _flip(dg, 8 * (len(dg) - 1))), (_flip(Y, rs.below(8 * cl)), sig, m, None),
              (_flip(Y, 8 * cl + rs.below(8 * cl)), sig, m, None)]
    Y, sig, m = base[1]
    r, s = sig[:ql], sig[ql:]
    for v in (0, q, q + 1):
        items += [(Y, _sc(v, ql) + s, m, None), (Y, r + _sc(v, ql), m, None)]
    # r + q names the same residue: a verifier that reduces r instead of refusing it would accept
    if int.from_bytes(r, "big") + q < 1 << (8 * ql):
        items.append((Y, _sc(int.from_bytes(r, "big") + q, ql) + s, m, None))
    Y, sig, m = base[2]
    P = pt_from(Y, cv)
    outside = [add(P, S["two"], cv), S["two"], S["full"]] + [S["low"][d] for d in sorted(S["low"])]
    items += [(pt_bytes(Z, cv), sig, m, None) for Z in outside]
    items += [(_sc(p, cl) + Y[cl:], sig, m, None), (b"\xff" * (2 * cl), sig, m, None), (bytes(2 * cl), sig, m, None)]
    if P[0] + p < 1 << (8 * cl):
        items.append((_sc(P[0] + p, cl) + Y[cl:], sig, m, None))
    cv["_verify"] = (b"".join(i[0] for i in items), b"".join(i[1] for i in items), b"".join(i[2] for i in items), 24,
                     b"".join(i[3] if i[3] is not None else H(i[2]).digest() for i in items), [i[3] is None for i in items])
    return cv["_verify"]


def yfx_batch(cv):
    """abscissas: random (about half have no root), 0, 1, p - 1, the generator's, the point of order two's (both roots 0), and
    values >= p"""
    if "_yfx" in cv:
        return cv["_yfx"]
    p, cl = cv["p"], clen(cv)
    rs = Stream("yfx/" + cv["name"])
    xs = [rs.below(p) for _ in range(16)] + [0, 1, 2, p - 1, p - 2, cv["gx"], special_points(cv)["two"][0]]
    xs += [p, (1 << (8 * cl)) - 1]
    if cv["gx"] + p < 1 << (8 * cl):
        xs.append(cv["gx"] + p)
    cv["_yfx"] = b"".join(_sc(x, cl) for x in xs)
    return cv["_yfx"]


def field_batch(cv):
    """(a, b) lists for ec_fp_op_batch: 128 random pairs, crafted values against one another, pairs with a + b = p, p - 1 and
    2^(32 NW), differences that borrow through every word, products that are 0, 1 and -1, and 64 pairs of operands close to p
    (on a modulus that fills its words these make t = (a b + m p) / R overflow R in the Montgomery product)"""
    if "_field" in cv:
        return cv["_field"]
    p, nw = cv["p"], words(cv)
    nl = (pbits(cv) + 63) // 64
    rs = Stream("field/" + cv["name"])
    A = [rs.below(p) for _ in range(128)]
    B = [rs.below(p) for _ in range(128)]
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    for k in range(1, nw + 1):
        vals += [(1 << (32 * k)) % p, ((1 << (32 * k)) - 1) % p]
    vals += [(1 << (p.bit_length() - 1)) - 1, (1 << (32 * nw)) % p, (1 << (64 * nl)) % p, pow(1 << (32 * nw), 2, p), pow(1 << (64 * nl), 2, p)]
    vals = list(dict.fromkeys(vals))
    for i, v in enumerate(vals):
        A += [v, v, rs.below(p)]
        B += [vals[(i + 1) % len(vals)], v, v]
    for _ in range(8):
        a = rs.between(1, p)
        A += [a, a, a, a, a]
        B += [p - a, p - 1 - a, pow(a, -1, p), p - pow(a, -1, p), 0]
    if (1 << (32 * nw)) - p < p:      # a + b = 2^(32 NW): the addition's carry out of the top word
        for _ in range(4):
            a = rs.between((1 << (32 * nw)) - p + 1, p)
            A.append(a), B.append((1 << (32 * nw)) - a)
    for k in range(nw):               # a - b borrows out of word k and through every word above it
        a = rs.below(1 << (32 * k)) if k else 0
        b = a + 1 + (rs.below(1 << 31) << (32 * k))
        if b < p:
            A.append(a), B.append(b)
    A += [0, 0, 1 << (32 * (nw - 2))]
    B += [1, p - 1, (1 << (32 * (nw - 2))) + 1]
    # operands close to p.  Where p > 3/4 R, R = 2^(32 NW), the Montgomery product's t = (a b + m p) / R reaches R about every
    # other time: b is drawn again until it does, so that these 96 products are known to end in the carry word
    span, R = 1 << (p.bit_length() - 8), 1 << (32 * nw)
    mpinv = (-pow(p, -1, R)) % R
    for _ in range(96):
        a = p - 1 - rs.below(span)
        b = p - 1 - rs.below(span)
        while 4 * p > 3 * R and (a * b + (a * b * mpinv % R) * p) // R < R:
            b = p - 1 - rs.below(span)
        A.append(a), B.append(b)
    cv["_field"] = (A, B)
    return cv["_field"]


def py_field(cv, op, A, B):
    """ec_fp_op_batch in Python: 0 a b 2^(-64 nl), 1 add, 2 sub, 3 mul, 4 inverse of a (0 for a = 0, as x^(p - 2) gives)"""
    p = cv["p"]
    nl = (pbits(cv) + 63) // 64
    ri = pow(1 << (64 * nl), -1, p)
    f = {0: lambda a, b: a * b * ri % p, 1: lambda a, b: (a + b) % p, 2: lambda a, b: (a - b) % p, 3: lambda a, b: a * b % p,
         4: lambda a, b: pow(a, p - 2, p)}[op]
    return [f(a, b) for a, b in zip(A, B)]


def top_carry_count(cv, A, B):
    """in how many of the products a_i b_i the library's Montgomery multiplication (radix 2^(32 NW)) has t = (a b + m p) / R at or
    above R, so that only the carry word tells fe_cond_sub to subtract"""
    p, R = cv["p"], 1 << (32 * words(cv))
    mpinv = (-pow(p, -1, R)) % R
    n = 0
    for a, b in zip(A, B):
        m = a * b * mpinv % R
        n += (a * b + m * p) // R >= R
    return n


def sample(n, k=PY_ITEMS):
    """the indices (a) answers in a batch of n: at most k, spread evenly"""
    step = max(1, -(-n // k))
    return list(range(0, n, step))


# how many items of each batch the unmodified reference's answers are recorded for (the fixture stays small; the restatement
# oracle answers every item, and the CPU test ties the two together on the recorded ones)
REF_ITEMS = {"fixed/q": 12, "fixed/long": 4, "fixed/short": 4, "var/q": 24, "var/long": 4, "var/short": 4, "add": 14, "dbl": 8,
             "sign": 10, "yfx": 10}


def ref_items(cv, kind):
    """the indices of batch `kind` that the fixture holds the reference's answers for: an even spread, and by name the items the
    batch exists for (the point of order two and the points of small order as bases, the exceptional pairs, the refusals)"""
    if kind in ("add", "dbl"):
        A, _, exc = add_batch(cv)
        n = len(A) // (2 * clen(cv))
        extra = [exc, exc + 3, exc + 4, exc + 8, exc + 9] if kind == "add" else [exc, exc + 3]
    elif kind == "sign":
        n, extra = len(sign_batch(cv)[0]) // qlen(cv), [13, 16, 17, 18, 19]
    elif kind == "yfx":
        n = len(yfx_batch(cv)) // clen(cv)
        extra = [16, 22, 23, n - 1]               # x = 0, the abscissa of the point of order two, x = p, the last (x >= p)
    else:
        label, slen, sc, _ = [b for b in smul_batches(cv) if b[0] == kind][0]
        n = len(sc) // slen
        nb = 4 + len(special_points(cv)["low"])
        # var/q: 11 scalars per base; the order-two point with an odd scalar, every small-order base with an odd and an even one,
        # the first point that does not import
        extra = [11 * 3 + 8] + [11 * b + d for b in range(4, nb) for d in (8, 9)] + [11 * nb] if kind == "var/q" else [0, n - 1]
    return sorted(set(sample(n, REF_ITEMS[kind])) | {i for i in extra if 0 <= i < n})


def pack(idx, status, *outs):
    """what the fixture keeps of an answer: the status bytes of the items `idx`, and each output array's bytes of those among
    them that succeeded (an item's width is the array's length over the batch size)"""
    n = len(status)
    rec = {"st": bytes(status[i] for i in idx).hex()}
    for k, out in enumerate(outs):
        w = len(out) // n
        rec["out%d" % k] = b"".join(out[w * i:w * (i + 1)] for i in idx if status[i] == 0).hex()
    return rec


def sha(*parts):
    h = hashlib.sha256()
    for x in parts:
        h.update(x if isinstance(x, bytes) else repr(x).encode())
    return h.hexdigest()


def batch_hashes(cv):
    """a SHA-256 per batch family: the fixture records them beside the reference's answers to these very bytes"""
    out = {"smul": sha(*[x for b in smul_batches(cv) for x in (b[0].encode(), b[2], b[3] or b"G")]),
           "add": sha(*add_batch(cv)[:2]), "sign": sha(*[x for x in sign_batch(cv) if isinstance(x, bytes)]),
           "verify": sha(*verify_batch(cv)[:3], verify_batch(cv)[4]), "yfx": sha(yfx_batch(cv))}
    return out
