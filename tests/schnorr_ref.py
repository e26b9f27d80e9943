"""BIP0340 and ECFSDSA item by item, three ways: a Python-integer restatement of the verify and sign rules (hashlib), the
UNMODIFIED reference through ctypes (the symbols tests/sigfam_ref.py already reaches in oracle/_ref/libecc_ref.so, plus
ec_pub_key_import_from_buf for projective keys), and the crafted inputs of the tests.

The reference hashes the message itself, so an item is (message, hash name).  What the GPU entry points take is built here: a
slot `u32 length | hash input`, BIP0340: H(tag) || H(tag) || r || <blank: Y.x> || m, ECFSDSA: W.x || W.y || m -- the formats of
ec_schnorr_verify_msg_all_batch -- and, for signing, the same with the commitment left blank too.

BIP0340's nonce: the reference's `rand` hook is asked for a value below 2^(8 qlen) -- the AUX value -- and derives k from it
with two tagged hashes (sig/bip0340.c:237-294); ec_schnorr_sign_batch takes k itself, so bip0340_nonce restates the derivation and
the fixture keeps the aux value, the derived k and the signature."""
import ctypes as C

import numpy as np

import oracles as O
import sigfam_ref as SF

ECFSDSA, BIP0340 = 5, 20                           # libecc's ec_alg_type numbers
ECDSA = 1
SCHEMES = {"BIP0340": BIP0340, "ECFSDSA": ECFSDSA}
CURVES = ["SECP256K1", "SECP256R1", "BRAINPOOLP256R1", "SECP384R1", "SECP521R1", "WEI25519"]
HSIZE = {"SHA224": 28, "SHA256": 32, "SHA384": 48, "SHA512": 64}
HASH_TYPE = {"SHA224": 1, "SHA256": 2, "SHA384": 3, "SHA512": 4}
PAD_EDGES = (0, 1, 55, 56, 63, 64, 111, 112, 119, 120)    # total hash-input lengths are steered onto these residues (see pad_msgs)
AFF, PRJ = 0, 1
TAG_CHALLENGE, TAG_AUX, TAG_NONCE = b"BIP0340/challenge", b"BIP0340/aux", b"BIP0340/nonce"
BUF = SF.BUF

H = SF.H
rand_int = SF.rand_int
pt_bytes = SF.pt_bytes
_curve = SF._curve


# Jacobian double-and-add on Python integers: oracles.py_mul inverts at every step, which is minutes over this fixture
def _jdbl(P, a, p):
    X, Y, Z = P
    if not Y or not Z:
        return (1, 1, 0)
    S4 = 4 * X * Y * Y % p
    M = (3 * X * X + a * pow(Z, 4, p)) % p
    X3 = (M * M - 2 * S4) % p
    return (X3, (M * (S4 - X3) - 8 * pow(Y, 4, p)) % p, 2 * Y * Z % p)


def _jadd(P, Q, a, p):
    if not P[2]:
        return Q
    if not Q[2]:
        return P
    Z1s, Z2s = P[2] * P[2] % p, Q[2] * Q[2] % p
    U1, U2 = P[0] * Z2s % p, Q[0] * Z1s % p
    S1, S2 = P[1] * Z2s * Q[2] % p, Q[1] * Z1s * P[2] % p
    if U1 == U2:
        return _jdbl(P, a, p) if S1 == S2 else (1, 1, 0)
    Hh, R = (U2 - U1) % p, (S2 - S1) % p
    H2 = Hh * Hh % p
    H3, V = Hh * H2 % p, U1 * H2 % p
    X3 = (R * R - H3 - 2 * V) % p
    return (X3, (R * (V - X3) - S1 * H3) % p, Hh * P[2] * Q[2] % p)


def _aff(P, p):
    if not P[2]:
        return None
    zi = pow(P[2], -1, p)
    return (P[0] * zi * zi % p, P[1] * zi * zi * zi % p)


def py_mul(k, P, a, p):
    """[k]P for an affine P or None, k >= 0: affine, or None for the point at infinity"""
    if P is None:
        return None
    R, B = (1, 1, 0), (P[0], P[1], 1)
    while k:
        if k & 1:
            R = _jadd(R, B, a, p)
        B = _jdbl(B, a, p)
        k >>= 1
    return _aff(R, p)


def py_add(P, Q, a, p):
    J = lambda T: (1, 1, 0) if T is None else (T[0], T[1], 1)
    return _aff(_jadd(J(P), J(Q), a, p), p)


def hashes_for(curve):
    """SHA-256 everywhere; on three curves the other sizes, so that hsize < qlen (SHA-224 / 256 / 384 on SECP521R1, SHA-256 on
    SECP384R1), = qlen (SHA-256 on the 256-bit curves, SHA-384 on SECP384R1) and > qlen (SHA-384 / 512 on SECP256K1, SHA-512 on
    SECP384R1) all occur"""
    return {"SECP256K1": ["SHA256", "SHA224", "SHA384", "SHA512"], "SECP384R1": ["SHA256", "SHA384", "SHA512"],
            "SECP521R1": ["SHA256", "SHA224", "SHA384", "SHA512"]}.get(curve, ["SHA256"])


def r_len(alg, cl):
    return cl if alg == BIP0340 else 2 * cl


def fixed_len(alg, hash_name, cl):
    return 2 * HSIZE[hash_name] + 2 * cl if alg == BIP0340 else 2 * cl


def tagged(hash_name, tag):
    t = H(hash_name, tag)
    return t + t


def hash_input(alg, hash_name, cl, r, yx, msg):
    """the bytes the scheme hashes: r is the signature's commitment bytes, yx the key's x (BIP0340)"""
    if alg == BIP0340:
        return tagged(hash_name, TAG_CHALLENGE) + r + yx + msg
    return r + msg


def slot(alg, hash_name, cl, msg, stride, r=None, length=None, blank_fill=0):
    """a message slot: the commitment field holds r (verification, as ec_schnorr_verify_msg_all_batch takes it) or is blank
    (r None: signing); the key's x is always blank.  length: the length word, when it is not the honest one"""
    rl = r_len(alg, cl)
    body = hash_input(alg, hash_name, cl, bytes([blank_fill]) * rl if r is None else r, bytes([blank_fill]) * cl, msg)
    ln = len(body) if length is None else length
    assert 4 + len(body) <= stride
    return ln.to_bytes(4, "little") + body + bytes(stride - 4 - len(body))


def stride_for(alg, hash_name, cl, max_msg):
    return (4 + fixed_len(alg, hash_name, cl) + max_msg + 3) & ~3


# ---------------------------------------------------------------------------------------------------------------------
# the Python-integer restatement
# ---------------------------------------------------------------------------------------------------------------------
def import_key(curve, key, fmt):
    """ec_pub_key_import_from_aff_buf / ec_pub_key_import_from_buf: ("ok", (x, y)), ("inf", None) or None where the import fails"""
    p, a, b, q, G = _curve(curve)
    cl = O.clen(curve)
    if fmt == AFF:
        Y = SF.import_pub(curve, key)
        return None if Y is None else ("ok", Y)
    X, Yc, Z = (int.from_bytes(key[i * cl:(i + 1) * cl], "big") for i in range(3))
    if X >= p or Yc >= p or Z >= p or (Yc * Yc * Z - X * X * X - a * X * Z * Z - b * Z * Z * Z) % p:
        return None
    if Z == 0:
        return ("zero", None) if X == 0 and Yc == 0 else ("inf", None)   # (0 : 0 : 0) satisfies the equation and imports
    zi = pow(Z, -1, p)
    P = (X * zi % p, Yc * zi % p)
    if O.CURVES[curve]["order"] != q and py_mul(q, P, a, p) is not None:
        return None
    return ("ok", P)


def challenge(curve, alg, hash_name, r, yx, msg):
    q = O.CURVES[curve]["q"]
    return int.from_bytes(H(hash_name, hash_input(alg, hash_name, O.clen(curve), r, yx, msg)), "big") % q


def verify(curve, alg, hash_name, key, fmt, sig, msg):
    """0 accept / 1 reject"""
    p, a, b, q, G = _curve(curve)
    cl, ql = O.clen(curve), O.qlen(curve)
    rl = r_len(alg, cl)
    K = import_key(curve, key, fmt)
    if K is None:
        return 1
    r, s = sig[:rl], int.from_bytes(sig[rl:], "big")
    rx = int.from_bytes(r[:cl], "big")
    if alg == BIP0340:
        if K[0] != "ok" or rx >= p or s >= q:
            return 1
        Y = K[1]
        e = challenge(curve, alg, hash_name, r, Y[0].to_bytes(cl, "big"), msg)
        if Y[1] & 1:
            Y = (Y[0], p - Y[1])
        R = py_add(py_mul(s, G, a, p), py_mul(-e % q, Y, a, p), a, p)
        return 0 if R is not None and not (R[1] & 1) and R[0] == rx else 1
    ry = int.from_bytes(r[cl:], "big")
    if rx >= p or ry >= p or (ry * ry - rx * rx * rx - a * rx - b) % p or not 0 < s < q:
        return 1
    if K[0] == "zero":
        return 1                                                      # prj_pt_mul of (0 : 0 : 0) fails (recorded: key_infinity)
    e = challenge(curve, alg, hash_name, r, b"", msg)
    eY = None if K[0] == "inf" else py_mul(-e % q, K[1], a, p)      # the key is used as it is: at infinity it adds nothing
    W = py_add(py_mul(s, G, a, p), eY, a, p)
    return 0 if W is not None and W == (rx, ry) else 1


def key_ok(alg, q, x):
    """what ec_key_pair_import_from_priv_key_buf and the scheme's signing accept (recorded: family x_edge)"""
    return 0 < x < q if alg == BIP0340 else x < q       # ECFSDSA signs with x = 0 (s = k)


def bip0340_nonce(curve, hash_name, x, aux, msg):
    """k = H_nonce(t || Y.x || m) mod q with t = d XOR H_aux(aux) over min(qlen, hsize) leading bytes (sig/bip0340.c:237-294); d is
    the private key AFTER the flip by the parity of Y.y"""
    p, a, b, q, G = _curve(curve)
    cl, ql = O.clen(curve), O.qlen(curve)
    Y = py_mul(x, G, a, p)
    d = q - x if Y[1] & 1 else x
    hs = HSIZE[hash_name]
    mask = H(hash_name, tagged(hash_name, TAG_AUX) + aux.to_bytes(ql, "big"))
    db = d.to_bytes(ql, "big")
    if ql > hs:
        t = bytes(u ^ v for u, v in zip(db[:hs], mask)) + db[hs:]
    else:
        t = bytes(u ^ v for u, v in zip(mask[:ql], db)) + mask[ql:]
    return int.from_bytes(H(hash_name, tagged(hash_name, TAG_NONCE) + t + Y[0].to_bytes(cl, "big") + msg), "big") % q


def sign(curve, alg, hash_name, x, k, msg, pub=None):
    """(status, signature bytes) as ec_schnorr_sign_batch returns them; pub: the affine key bytes the caller supplies (BIP0340), or
    None for [x]G"""
    p, a, b, q, G = _curve(curve)
    cl, ql = O.clen(curve), O.qlen(curve)
    bad = (1, bytes(r_len(alg, cl) + ql))
    if not key_ok(alg, q, x) or not 0 < k < q:
        return bad
    R = py_mul(k, G, a, p)
    if alg == ECFSDSA:
        r = pt_bytes(curve, R)
        s = (k + challenge(curve, alg, hash_name, r, b"", msg) * x) % q
        return (0, r + s.to_bytes(ql, "big")) if s else bad
    if pub is None:
        Y = py_mul(x, G, a, p)
    else:
        Y = (int.from_bytes(pub[:cl], "big"), int.from_bytes(pub[cl:], "big"))
        if Y[0] >= p or Y[1] >= p or (Y[1] * Y[1] - Y[0] ** 3 - a * Y[0] - b) % p:
            return bad
    d = q - x if Y[1] & 1 else x
    kk = q - k if R[1] & 1 else k
    r = R[0].to_bytes(cl, "big")
    s = (kk + challenge(curve, alg, hash_name, r, Y[0].to_bytes(cl, "big"), msg) * d) % q
    return 0, r + s.to_bytes(ql, "big")


# ---------------------------------------------------------------------------------------------------------------------
# the reference through ctypes
# ---------------------------------------------------------------------------------------------------------------------
def ref_verify(curve, alg, hash_name, key, fmt, sig, msg):
    """ec_pub_key_import_from_aff_buf / ec_pub_key_import_from_buf + ec_verify: 0 / -1"""
    L, params = SF.ref_params(curve)
    L.ec_pub_key_import_from_buf.argtypes = L.ec_pub_key_import_from_aff_buf.argtypes
    kb = C.create_string_buffer(BUF)
    imp = L.ec_pub_key_import_from_aff_buf if fmt == AFF else L.ec_pub_key_import_from_buf
    if imp(kb, params, key, len(key), alg) != 0:
        return -1
    return -1 if L.ec_verify(sig, len(sig), kb, msg, len(msg), alg, O.HASH_IDS[hash_name], None, 0) != 0 else 0


def ref_sign(curve, alg, hash_name, x, v, msg):
    """ec_key_pair_import_from_priv_key_buf + _ec_sign whose `rand` hook returns v -- ECFSDSA: the nonce k (asked below q), BIP0340:
    the aux value (asked below 2^(8 qlen)): (ret, signature bytes or None); ret -2: the key pair import failed"""
    L, params = SF.ref_params(curve)
    ql, cl = O.qlen(curve), O.clen(curve)
    kp = C.create_string_buffer(BUF)
    if L.ec_key_pair_import_from_priv_key_buf(kp, params, x.to_bytes(ql, "big"), ql, alg) != 0:
        return -2, None
    calls = [0]
    vb = v.to_bytes(ql + 1, "big")

    def hook(out, bound):
        calls[0] += 1
        if calls[0] > 1:
            return -1
        cmp = C.c_int(0)
        if L.nn_init_from_buf(out, vb, len(vb)) != 0 or L.nn_cmp(out, bound, C.byref(cmp)) != 0:
            return -1
        return -1 if cmp.value >= 0 else 0

    cb = SF.RAND_FN(hook)
    sl = r_len(alg, cl) + ql
    sig = C.create_string_buffer(sl)
    ret = L._ec_sign(sig, sl, kp, msg, len(msg), cb, alg, O.HASH_IDS[hash_name], None, 0)
    return (0, sig.raw[:sl]) if ret == 0 else (-1, None)


DELTA = ("hash", "msg", "key", "fmt", "r", "s", "x", "v")   # fields the fixture file leaves out where the previous item has the same


def pattern_msg(n):
    return bytes((7 * i + 3) & 0xFF for i in range(n))


def load_fixture(path):
    """tests/golden/schnorr_items.json with the left-out fields put back"""
    import json
    with open(path) as f:
        fx = json.load(f)
    for per in fx.values():
        for d in per.values():
            for items in d.values():
                for j, it in enumerate(items):
                    if "msgpat" in it:
                        it["msg"] = pattern_msg(it.pop("msgpat")).hex()
                    if j:
                        for k in DELTA:
                            if k not in it and k in items[j - 1]:
                                it[k] = items[j - 1][k]
    return fx


# ---------------------------------------------------------------------------------------------------------------------
# crafted inputs
# ---------------------------------------------------------------------------------------------------------------------
def prj_bytes(curve, P, z):
    """(x z : y z : z) as X || Y || Z; P None: the point at infinity (0 : 1 : 0)"""
    p, cl = O.CURVES[curve]["p"], O.clen(curve)
    if P is None:
        return bytes(cl) + (1).to_bytes(cl, "big") + bytes(cl)
    return b"".join((c % p).to_bytes(cl, "big") for c in (P[0] * z, P[1] * z, z))


def pad_msgs(alg, hash_name, cl):
    """messages whose whole hash input ends on each of PAD_EDGES modulo the hash's block size (SHA-224 / 256: 64, SHA-384 / 512: 128)"""
    block = 64 if HSIZE[hash_name] <= 32 else 128
    fl = fixed_len(alg, hash_name, cl)
    return [pattern_msg((edge - fl) % block) for edge in PAD_EDGES if edge < block]


def verify_families(curve, alg, rng):
    """{family: [(hash name, message, key bytes, key format, signature bytes)]}"""
    p, a, b, q, G = _curve(curve)
    ql, cl = O.qlen(curve), O.clen(curve)
    rl = r_len(alg, cl)
    hs = hashes_for(curve)
    h0 = hs[0]
    qtop, ctop = (1 << (8 * ql)) - 1, (1 << (8 * cl)) - 1
    fam = {}

    def rmsg():
        return rng.integers(0, 256, size=int(rng.integers(1, 48)), dtype=np.uint8).tobytes()

    def rk():
        return 1 + rand_int(rng, q - 1)

    def keypair(odd=None):
        while True:
            x = rk()
            Y = py_mul(x, G, a, p)
            if odd is None or bool(Y[1] & 1) == odd:
                return x, pt_bytes(curve, Y)

    def honest(h, x, msg=None, want_r_odd=None):
        while True:
            m, k = rmsg() if msg is None else msg, rk()
            if want_r_odd is not None and bool(py_mul(k, G, a, p)[1] & 1) != want_r_odd:
                continue
            st, sig = sign(curve, alg, h, x, k, m)
            if st == 0:
                return m, sig

    def sb(r, s):
        return r + s.to_bytes(ql, "big")

    x, pub = keypair()
    X, Y = int.from_bytes(pub[:cl], "big"), int.from_bytes(pub[cl:], "big")
    fam["honest"] = [(h, *honest(h, x)) for h in hs]
    fam["honest"] = [(h, m, pub, AFF, sig) for h, m, sig in fam["honest"]]
    if curve == "SECP256K1":   # both block sizes
        fam["pad_edges"] = [(h, m, pub, AFF, honest(h, x, m)[1]) for h in ("SHA256", "SHA512") for m in pad_msgs(alg, h, cl)]
    msg, sig = honest(h0, x)
    r0, s0 = sig[:rl], int.from_bytes(sig[rl:], "big")
    fam["tampered"] = [(h0, msg, pub, AFF, sb(r0, s0 % (q - 1) + 1)), (h0, msg + b"!", pub, AFF, sig), (h0, msg, keypair()[1], AFF, sig),
                       (h0, msg, pub, AFF, sb(bytes([r0[0] ^ 1]) + r0[1:], s0))]
    fam["s_range"] = [(h0, msg, pub, AFF, sb(r0, s)) for s in (0, 1, q - 1, q, min(qtop, q + 1), qtop)]
    # the commitment: x >= p, x = p - 1, an x that is no abscissa (BIP0340) / a point off the curve, y >= p, y negated (ECFSDSA)
    rx0 = int.from_bytes(r0[:cl], "big")
    nonab = next(v for v in range(2, 1000) if SF.sqrt_mod(v ** 3 + a * v + b, p) is None)
    rxs = [min(p, ctop), min(rx0 + p, ctop) if rx0 + p <= ctop else min(p + 1, ctop), p - 1, nonab]
    fam["r_range"] = [(h0, msg, pub, AFF, sb(v.to_bytes(cl, "big") + r0[cl:], s0)) for v in rxs]
    if alg == ECFSDSA:
        ry0 = int.from_bytes(r0[cl:], "big")
        fam["w_bad"] = [(h0, msg, pub, AFF, sb(r0[:cl] + v.to_bytes(cl, "big"), s0))
                        for v in (min(p, ctop), min(ry0 + p, ctop) if ry0 + p <= ctop else min(p + 1, ctop), (ry0 + 1) % p, p - ry0)]
    # keys: odd and even y, also with the commitment's y odd and even
    fam["key_parity"] = []
    for odd in (True, False):
        xx, pb = keypair(odd)
        for r_odd in (True, False):
            m2, sg = honest(h0, xx, want_r_odd=r_odd)
            fam["key_parity"].append((h0, m2, pb, AFF, sg))
    bad = [pub[:cl] + ((Y + 1) % p).to_bytes(cl, "big"), bytes(2 * cl), pub[:cl] + min(Y + p, ctop).to_bytes(cl, "big"),
           (X + p if X + p <= ctop else min(p, ctop)).to_bytes(cl, "big") + pub[cl:]]
    fam["key_not_importable"] = [(h0, msg, k, AFF, sig) for k in bad]
    if O.CURVES[curve]["order"] != q:
        T = SF.small_order_point(curve, rng)
        fam["key_small_order"] = [(h0, msg, pt_bytes(curve, T), AFF, sig), (h0, msg, prj_bytes(curve, T, 5), PRJ, sig)]
        fam["key_torsion"] = [(h0, msg, pt_bytes(curve, py_add((X, Y), T, a, p)), AFF, sig)]
    # projective keys: Z = 1, Z != 1 (accepted), off the curve, a coordinate >= p, the point at infinity, (0 : 0 : 0)
    z = 2 + rand_int(rng, p - 2)
    fam["key_projective"] = [(h0, msg, prj_bytes(curve, (X, Y), 1), PRJ, sig), (h0, msg, prj_bytes(curve, (X, Y), z), PRJ, sig),
                             (h0, msg, prj_bytes(curve, (X, Y + 1), z), PRJ, sig),
                             (h0, msg, pub + min(p, ctop).to_bytes(cl, "big"), PRJ, sig)]
    fam["key_infinity"] = [(h0, msg, prj_bytes(curve, None, 1), PRJ, sig), (h0, msg, bytes(3 * cl), PRJ, sig)]
    if alg == ECFSDSA:
        # a key at infinity with W = [s]G: the sum is [s]G whatever e is
        s1 = rk()
        w1 = pt_bytes(curve, py_mul(s1, G, a, p))
        fam["key_infinity"] += [(h0, msg, prj_bytes(curve, None, 1), PRJ, sb(w1, s1)), (h0, msg, bytes(3 * cl), PRJ, sb(w1, s1))]
    # the other scheme's signature, and an ECDSA signature, offered under this one
    other = ECFSDSA if alg == BIP0340 else BIP0340
    so = sign(curve, other, h0, x, rk(), msg)[1]
    k = rk()
    er = py_mul(k, G, a, p)[0] % q
    es = pow(k, -1, q) * (int.from_bytes(H(h0, msg)[:ql], "big") + er * x) % q
    ecdsa = er.to_bytes(ql, "big") + es.to_bytes(ql, "big")
    fam["foreign_scheme"] = [(h0, msg, pub, AFF, (so + bytes(rl + ql))[:rl + ql]), (h0, msg, pub, AFF, (ecdsa + bytes(rl + ql))[:rl + ql])]
    # exceptional pairs, Y = G (x = 1; G.y even or odd as it comes: the lift may turn Y into -G): [s]G = +-[q - e]Y', s chosen after e
    gb = pt_bytes(curve, G)
    sign_g = -1 if (alg == BIP0340 and G[1] & 1) else 1    # Y' = sign_g G
    exc = []
    for tries in range(64):
        m2 = rmsg()
        # a commitment that is a valid r / W: [t]G for some t
        Wt = py_mul(rk(), G, a, p)
        r = pt_bytes(curve, Wt)[:rl]
        e = challenge(curve, alg, h0, r, gb[:cl], m2)
        ne = -e % q
        if ne == 0:
            continue
        # [s]G + [ne]Y' = [s + sign_g ne]G:  s = sign_g ne: a doubling;  s = -sign_g ne: the point at infinity
        exc = [(h0, m2, gb, AFF, sb(r, sign_g * ne % q)), (h0, m2, gb, AFF, sb(r, -sign_g * ne % q))]
        break
    # ... and an ACCEPTED doubling: the commitment is [2 s]G itself only if it was chosen before e, which it cannot be; so the
    # accepted exceptional items are those with s = 0 (BIP0340: R = [q - e]Y' alone), found by trying messages
    fam["exceptional_pairs"] = exc
    if alg == BIP0340:
        fam["s_zero"] = [(h0, msg, gb, AFF, sb(r0, 0)), (h0, msg, pub, AFF, sb(r0, 0))]
    return fam


def sign_families(curve, alg, rng):
    """{family: [(hash name, message, x, v)]}; v is what the reference's `rand` hook returns: k (ECFSDSA) or aux (BIP0340)"""
    p, a, b, q, G = _curve(curve)
    ql, cl = O.qlen(curve), O.clen(curve)
    hs = hashes_for(curve)
    h0 = hs[0]
    fam = {}

    def rmsg():
        return rng.integers(0, 256, size=int(rng.integers(1, 48)), dtype=np.uint8).tobytes()

    def rk():
        return 1 + rand_int(rng, q - 1)

    def rv():
        return rk() if alg == ECFSDSA else rand_int(rng, 1 << (8 * ql))

    def nonce(h, x, v, m):
        return v if alg == ECFSDSA else bip0340_nonce(curve, h, x, v, m)

    fam["honest"] = [(h, rmsg(), rk(), rv()) for h in hs]
    if curve == "SECP256K1":
        fam["pad_edges"] = [(h, m, rk(), rv()) for h in ("SHA256", "SHA512") for m in pad_msgs(alg, h, cl)[::3]]
    # every combination of the parities of Y.y and R.y
    par = []
    for y_odd in (True, False):
        while True:
            x = rk()
            if bool(py_mul(x, G, a, p)[1] & 1) == y_odd:
                break
        for r_odd in (True, False):
            while True:
                m, v = rmsg(), rv()
                if bool(py_mul(nonce(h0, x, v, m), G, a, p)[1] & 1) == r_odd:
                    break
            par.append((h0, m, x, v))
    fam["parity"] = par
    m, x0, v0 = rmsg(), rk(), rv()
    top = (1 << (8 * ql)) - 1
    fam["x_edge"] = [(h0, m, x, v0) for x in (0, 1, q - 1, q, min(top, q + 1))]
    if alg == ECFSDSA:
        fam["k_edge"] = [(h0, m, x0, k) for k in (0, 1, q - 1, q, min(top, q + 1))]
    else:
        fam["aux_edge"] = [(h0, m, x0, v) for v in (0, top)]
    return fam
