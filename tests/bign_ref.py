"""BIGN / DBIGN (STB 34.101.45) three ways: a pure-Python BelT-hash (STB 34.101.31) with a Python-integer restatement of the sign
and verify rules, the UNMODIFIED reference through ctypes (the symbols tests/sigfam_ref.py already reaches in
oracle/_ref/libecc_ref.so, plus belt_hash), and the crafted inputs of the tests.

The reference hashes the message itself, so an item is (message, hash name, OID).  What the GPU entry points take is built by
device_input: the digest H(m) for hash_type 0, or a message slot `u32 length | message` for a hash the device computes.
Everything BIGN writes is little-endian: s0, s1, the digest read as a number, the coordinates of W in the hash input."""
import ctypes as C
import hashlib

import numpy as np

import oracles as O
import sigfam_ref as SF

BIGN, DBIGN = 18, 19                               # libecc's ec_alg_type numbers
HASH_BELT = 16                                     # libecc's hash_alg_type number of BELT_HASH
HASH_IDS = dict(O.HASH_IDS, BELT=HASH_BELT)
HSIZE = {"SHA224": 28, "SHA256": 32, "SHA384": 48, "SHA512": 64, "BELT": 32}
CURVES = ["BIGN256V1", "BIGN384V1", "BIGN512V1", "SECP256R1", "SECP521R1", "SECP224K1", "WEI25519"]
HASHES = ["BELT", "SHA256", "SHA512", "SHA224"]
# the OID of belt-hash (1.2.112.0.2.0.34.101.31.81) in DER, as the standard's test vectors carry it
OID_BELT = bytes.fromhex("06092A7000020022651F51")
MSG_LENS = (0, 1, 31, 32, 33, 200)

rand_int = SF.rand_int
pt_bytes = SF.pt_bytes
import_pub = SF.import_pub
_curve = SF._curve

# ---------------------------------------------------------------------------------------------------------------------
# BelT (STB 34.101.31), from the standard's definitions, on Python integers
# ---------------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def _table():
    rows = ["B194BAC80A08F53B366D008E584A5DE4", "8504FA9D1BB6C7AC252E72C202FDCE0D", "5BE3D61217B96181FE6786AD716B890B",
            "5CB0C0FF33C356B835C405AED8E07F99", "E12BDC1AE28257EC703FCCF095EE8DF1", "C1AB76389FE678CAF7C6F860D5BB9C4F",
            "F33C657B637C306ADD4EA7799EB23D31", "3E98B56E27D3BCCF591E181F4C5AB793", "E9DEE72C8F0C0FA62DDB49F46F739647",
            "06075316ED247A3739CBA38303A98BF6", "92BD9B1CE5D141015445FBC95E4D0EF2", "682080AA227D642F2687F93490405511",
            "BE32971343FC9A48A02A885F194B09A1", "7ECDA4D01544AF8CA58450BF66D2E88A", "A2D7465242A8DFB36974C551EB232921",
            "D4EFD9B43A622875911410EA776CDA1D"]
    t = bytes.fromhex("".join(rows))
    assert len(t) == 256 and sorted(t) == list(range(256))   # H is a permutation
    return t


BELT_H = _table()


def _g(u, r):
    t = BELT_H[u & 0xff] | (BELT_H[(u >> 8) & 0xff] << 8) | (BELT_H[(u >> 16) & 0xff] << 16) | (BELT_H[u >> 24] << 24)
    return ((t << r) | (t >> (32 - r))) & M32


def belt_encrypt(block, key):
    """F_key(block): 16 and 32 bytes"""
    a, b, c, d = (int.from_bytes(block[4 * j:4 * j + 4], "little") for j in range(4))
    th = [int.from_bytes(key[4 * j:4 * j + 4], "little") for j in range(8)]
    K = [th[j % 8] for j in range(56)]
    for i in range(1, 9):
        k = K[7 * (i - 1):7 * i]
        b ^= _g((a + k[0]) & M32, 5)
        c ^= _g((d + k[1]) & M32, 21)
        a = (a - _g((b + k[2]) & M32, 13)) & M32
        e = _g((b + c + k[3]) & M32, 21) ^ i
        b = (b + e) & M32
        c = (c - e) & M32
        d = (d + _g((c + k[4]) & M32, 13)) & M32
        b ^= _g((a + k[5]) & M32, 21)
        c ^= _g((d + k[6]) & M32, 5)
        a, b = b, a
        c, d = d, c
        b, c = c, b
    return b"".join(v.to_bytes(4, "little") for v in (b, d, a, c))


def _xor(x, y):
    return bytes(p ^ q for p, q in zip(x, y))


def _sigma1(u):
    u34 = _xor(u[32:48], u[48:64])
    return _xor(belt_encrypt(u34, u[:32]), u34)


def _sigma2(u):
    t = _sigma1(u)
    return _xor(belt_encrypt(u[:16], t + u[48:64]), u[:16]) + _xor(belt_encrypt(u[16:32], _xor(t, b"\xff" * 16) + u[32:48]), u[16:32])


def belt_hash(msg):
    s, h = bytes(16), BELT_H[:32]
    for off in range(0, len(msg), 32):
        X = msg[off:off + 32].ljust(32, b"\0")
        s, h = _xor(s, _sigma1(X + h)), _sigma2(X + h)
    return _sigma2((8 * len(msg)).to_bytes(16, "little") + s + h)


def H(hash_name, data):
    return belt_hash(data) if hash_name == "BELT" else hashlib.new(O.HASHLIB[hash_name], data).digest()


def fast_mul(k, P, a, p):
    """[k]P as an affine point or None, as oracles.py_mul gives it, on Jacobian coordinates with one inversion at the end (the
    affine ladder of oracles.py inverts at every step, which is slow on the 512- and 521-bit curves)"""
    if P is None or k == 0:
        return None
    X1, Y1 = P
    R = None
    for bit in bin(k)[2:]:
        if R is not None:
            X, Y, Z = R
            if Y == 0:
                R = None
            else:
                S = 4 * X * Y * Y % p
                M = (3 * X * X + a * pow(Z, 4, p)) % p
                X3 = (M * M - 2 * S) % p
                R = (X3, (M * (S - X3) - 8 * pow(Y, 4, p)) % p, 2 * Y * Z % p)
        if bit == "1":
            if R is None:
                R = (X1, Y1, 1)
            else:
                X, Y, Z = R
                Z2 = Z * Z % p
                U2, S2 = X1 * Z2 % p, Y1 * Z2 * Z % p
                H_, r = (U2 - X) % p, (S2 - Y) % p
                if H_ == 0:
                    if r == 0:
                        Q = O.py_add(P, P, a, p)      # the rare doubling inside an addition: through the affine formulas
                        R = None if Q is None else (Q[0], Q[1], 1)
                    else:
                        R = None
                else:
                    H2 = H_ * H_ % p
                    H3, V = H2 * H_ % p, X * H2 % p
                    X3 = (r * r - H3 - 2 * V) % p
                    R = (X3, (r * (V - X3) - Y * H3) % p, Z * H_ % p)
    if R is None or R[2] == 0:
        return None
    zi = pow(R[2], -1, p)
    return R[0] * zi * zi % p, R[1] * zi * zi * zi % p


def pattern_msg(n):
    """the fixed pattern of the BelT known answers and of the fixture's longer messages, named in the file by its length"""
    return bytes((11 * j + 5) & 0xff for j in range(n))


# ---------------------------------------------------------------------------------------------------------------------
# the Python-integer restatement
# ---------------------------------------------------------------------------------------------------------------------
def s0_len(curve):
    return O.qlen(curve) // 2


def sig_len(curve):
    return s0_len(curve) + O.qlen(curve)


def commit_t(curve, oid, W, dg):
    """t: the first min(l, 32) bytes of belt-hash(OID || <LE(Wx) || LE(Wy)>_2l || digest), zero-padded to l bytes"""
    cl, l = O.clen(curve), s0_len(curve)
    w = (W[0].to_bytes(cl, "little") + W[1].to_bytes(cl, "little")).ljust(2 * l, b"\0")[:2 * l]
    return belt_hash(oid + w + dg)[:min(l, 32)].ljust(l, b"\0")


def front_end(curve, sig, dg):
    """(flag, u of G, v of Y)"""
    q, l = O.CURVES[curve]["q"], s0_len(curve)
    s0, s1 = int.from_bytes(sig[:l], "little"), int.from_bytes(sig[l:], "little")
    if s1 >= q:
        return 1, 0, 0
    return 0, (s1 + int.from_bytes(dg, "little")) % q, (s0 + (1 << (8 * l))) % q


def verify_digest(curve, oid, pub, sig, dg):
    """0 accept / 1 reject, from the digest of the message"""
    p, a, b, q, G = _curve(curve)
    l = s0_len(curve)
    Y = import_pub(curve, pub)
    if Y is None:
        return 1
    flag, u, v = front_end(curve, sig, dg)
    if flag:
        return 1
    W = O.py_add(fast_mul(u, G, a, p), fast_mul(v, Y, a, p), a, p)
    if W is None:
        return 1
    return 0 if commit_t(curve, oid, W, dg) == sig[:l] else 1


def verify(curve, hash_name, oid, pub, sig, msg):
    return verify_digest(curve, oid, pub, sig, H(hash_name, msg))


def sign_s1(curve, x, k, dg, s0):
    q, l = O.CURVES[curve]["q"], s0_len(curve)
    return (k - int.from_bytes(dg, "little") - (int.from_bytes(s0, "little") + (1 << (8 * l))) * x) % q


def sign_digest(curve, oid, x, k, dg):
    """(status, signature bytes) as ec_bign_sign_batch returns them.  What the recording shows (tests/golden/bign.json): the key
    pair imports for x < q, x = 0 included (its public key [0]G is never read by the signer); the nonce hook fails for k >= q; k = 0
    fails: [0]G has no unique affine form."""
    p, a, b, q, G = _curve(curve)
    bad = (1, bytes(sig_len(curve)))
    if not x < q or not 0 < k < q:
        return bad
    s0 = commit_t(curve, oid, fast_mul(k, G, a, p), dg)
    return 0, s0 + sign_s1(curve, x, k, dg, s0).to_bytes(O.qlen(curve), "little")


def sign(curve, hash_name, oid, x, k, msg):
    return sign_digest(curve, oid, x, k, H(hash_name, msg))


# ---------------------------------------------------------------------------------------------------------------------
# the reference through ctypes
# ---------------------------------------------------------------------------------------------------------------------
def adata(oid, t=b""):
    """bign_set_adata's framing: two big-endian u16 lengths, the OID, then t (DBIGN's nonce generator alone reads t)"""
    return len(oid).to_bytes(2, "big") + len(t).to_bytes(2, "big") + oid + t


def ref_belt_hash(msg):
    L = C.CDLL(O.REF_SO)
    L.belt_hash.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p]
    out = C.create_string_buffer(32)
    assert L.belt_hash(msg, len(msg), out) == 0
    return out.raw


def ref_verify(curve, hash_name, oid, pub, sig, msg, alg=BIGN):
    """ec_pub_key_import_from_aff_buf + ec_verify: 0 / -1"""
    L, params = SF.ref_params(curve)
    key = C.create_string_buffer(SF.BUF)
    if L.ec_pub_key_import_from_aff_buf(key, params, pub, len(pub), alg) != 0:
        return -1
    ad = adata(oid)
    return -1 if L.ec_verify(sig, len(sig), key, msg, len(msg), alg, HASH_IDS[hash_name], ad, len(ad)) != 0 else 0


def ref_sign(curve, hash_name, oid, x, k, msg, alg=BIGN):
    """ec_key_pair_import_from_priv_key_buf + _ec_sign with the nonce k from the `rand` hook: (ret, signature bytes or None); ret
    -2: the key pair import failed.  The hook fails for k >= q, as in sigfam_ref.ref_sign."""
    L, params = SF.ref_params(curve)
    ql, sl = O.qlen(curve), sig_len(curve)
    kp = C.create_string_buffer(SF.BUF)
    if L.ec_key_pair_import_from_priv_key_buf(kp, params, x.to_bytes(ql, "big"), ql, alg) != 0:
        return -2, None
    calls = [0]
    kb = k.to_bytes(ql + 1, "big")

    def hook(out, q):
        calls[0] += 1
        if calls[0] > 1:
            return -1
        cmp = C.c_int(0)
        if L.nn_init_from_buf(out, kb, len(kb)) != 0 or L.nn_cmp(out, q, C.byref(cmp)) != 0:
            return -1
        return -1 if cmp.value >= 0 else 0

    cb = SF.RAND_FN(hook)
    sig = C.create_string_buffer(sl)
    ad = adata(oid)
    ret = L._ec_sign(sig, sl, kp, msg, len(msg), cb, alg, HASH_IDS[hash_name], ad, len(ad))
    return (0, sig.raw[:sl]) if ret == 0 else (-1, None)


# ---------------------------------------------------------------------------------------------------------------------
# what the entry points take
# ---------------------------------------------------------------------------------------------------------------------
def slot(msg, stride, length=None):
    ln = len(msg) if length is None else length
    assert 4 + len(msg) <= stride and stride % 4 == 0
    return ln.to_bytes(4, "little") + msg + bytes(stride - 4 - len(msg))


def stride_for(max_msg):
    return (4 + max_msg + 3) & ~3


def device_input(hash_name, msg, stride=None):
    """the digest H(m) (stride None: hash_type 0) or the message slot of `stride` bytes (hash_type HASH_IDS[hash_name])"""
    return H(hash_name, msg) if stride is None else slot(msg, stride)


# fields the fixture file leaves out where the previous item has the same
DELTA = ("family", "hash", "oid", "msg", "pub", "s0", "s1", "x", "k")


def load_fixture(path):
    """tests/golden/bign.json with the left-out fields put back: {"belt": [[length, digest hex]], curve: {"verify", "sign"}}"""
    import json
    with open(path) as f:
        fx = json.load(f)
    for curve, d in fx.items():
        if curve == "belt":
            continue
        for items in d.values():
            for j, i in enumerate(items):
                if "msgpat" in i:
                    i["msg"] = pattern_msg(i.pop("msgpat")).hex()
                for k in DELTA:
                    if j and k not in i and k in items[j - 1]:
                        i[k] = items[j - 1][k]
                if "s0" in i:
                    i["sig"] = i["s0"] + i["s1"]
    return fx


# ---------------------------------------------------------------------------------------------------------------------
# crafted inputs
# ---------------------------------------------------------------------------------------------------------------------
def hashes_for(curve):
    """BelT and SHA-256 everywhere; SHA-512 (a digest longer than q on the short curves) and SHA-224 on a short and a long curve"""
    return HASHES if curve in ("BIGN256V1", "SECP521R1", "SECP224K1") else ["BELT", "SHA256", "SHA512"]


def verify_families(curve, rng):
    """{family: [(hash name, OID, message, public key bytes, signature bytes)]}"""
    p, a, b, q, G = _curve(curve)
    ql, cl, l = O.qlen(curve), O.clen(curve), s0_len(curve)
    hs = hashes_for(curve)
    oid = OID_BELT
    fam = {}

    def rmsg(n=None):
        return rng.integers(0, 256, size=int(rng.integers(1, 48)) if n is None else n, dtype=np.uint8).tobytes()

    def rk():
        return 1 + rand_int(rng, q - 1)

    def honest(h, x, pub, msg=None, o=oid):
        m = rmsg() if msg is None else msg
        st, sig = sign(curve, h, o, x, rk(), m)
        assert st == 0
        return h, o, m, pub, sig

    def le(v, n):
        return v.to_bytes(n, "little")

    def flip(bs, i, bit=1):
        return bs[:i] + bytes([bs[i] ^ bit]) + bs[i + 1:]

    x = rk()
    Y = fast_mul(x, G, a, p)
    pub = pt_bytes(curve, Y)
    fam["honest"] = [honest(h, x, pub) for h in hs]
    h, _, msg, _, sig = honest(hs[0], x, pub)
    s0b, s1b = sig[:l], sig[l:]
    dg = H(h, msg)
    hbar = int.from_bytes(dg, "little") % q
    fam["s0_bit"] = [(h, oid, msg, pub, flip(sig, 0)), (h, oid, msg, pub, flip(sig, l - 1, 0x80))]
    fam["s1_bit"] = [(h, oid, msg, pub, flip(sig, l)), (h, oid, msg, pub, flip(sig, l + ql - 1, 0x01))]
    top = (1 << (8 * ql)) - 1

    def with_s1(target):
        """an honest signature whose s1 is `target`: the nonce first, then the key that makes it so (x = (k - hbar - s1) / v)"""
        k = rk()
        t = commit_t(curve, oid, fast_mul(k, G, a, p), dg)
        xx = (k - hbar - target) * pow((int.from_bytes(t, "little") + (1 << (8 * l))) % q, -1, q) % q
        return h, oid, msg, pt_bytes(curve, fast_mul(xx, G, a, p)), t + le(target, ql)

    # s1 = 0 and q - 1 on signatures that are honest for their (crafted) keys: accepted; q and the largest value: refused by the range
    fam["s1_range"] = [with_s1(0), with_s1(q - 1), (h, oid, msg, pub, s0b + le(0, ql)), (h, oid, msg, pub, s0b + le(q, ql)),
                       (h, oid, msg, pub, s0b + le(top, ql))]
    hh_, oo_, mm_, pp_, ss_ = with_s1(5)
    fam["s1_range"].append((hh_, oo_, mm_, pp_, ss_[:l] + le(q + 5, ql)) if q + 5 <= top else (hh_, oo_, mm_, pp_, ss_))
    fam["s0_const"] = [(h, oid, msg, pub, bytes(l) + s1b), (h, oid, msg, pub, b"\xff" * l + s1b)]

    # crafted from the private key: u = 0 (W' = [v]Y alone), W' at infinity, the doubling [u]G = [v]Y.  For each, s0 is tried until
    # (where it can) the hash agrees: with u = 0 and with the doubling W' is a known point, so t is computed first and s0 = t is
    # consistent only if v(t) reproduces W' -- it cannot be forced; the item is recorded as the reference judges it.
    def crafted(kind, hh):
        m2 = rmsg()
        d2 = H(hh, m2)
        hb = int.from_bytes(d2, "little") % q
        s0 = rng.integers(0, 256, size=l, dtype=np.uint8).tobytes()
        v = (int.from_bytes(s0, "little") + (1 << (8 * l))) % q
        if kind == "u_zero":
            s1 = -hb % q
        elif kind == "w_infinity":
            s1 = (-v * x - hb) % q            # u = -v x
        else:
            s1 = (v * x - hb) % q             # u = v x
        return hh, oid, m2, pub, s0 + le(s1, ql)

    # u = 0 with an ACCEPTED verdict: k = v x with v = s0 + 2^(8l) needs s0 = t(W) for W = [v x]G -- a fixed point of the hash.
    # Instead the signer is run backwards: choose k, W = [k]G, s0 = t, and find the message whose digest has hbar = k - v x ...
    # which inverts the hash.  So u = 0 is accepted only at the level of the entry point that takes the digest from the caller
    # (u_zero_accepted below); through the reference these items are rejected ones.
    fam["u_zero"] = [crafted("u_zero", hh) for hh in hs]
    fam["w_infinity"] = [crafted("w_infinity", hh) for hh in hs]
    fam["doubling"] = [crafted("doubling", hh) for hh in hs]
    if l > 32:
        hs_, o_, m_, p_, sg = honest(hs[0], x, pub)
        fam["s0_byte32"] = [(hs_, o_, m_, p_, sg), (hs_, o_, m_, p_, flip(sg, 32)), (hs_, o_, m_, p_, flip(sg, 32, 0x80))]
    X, Yy = Y
    ctop = (1 << (8 * cl)) - 1
    fam["key_off_curve"] = [(h, oid, msg, flip(pub, 0), sig), (h, oid, msg, flip(pub, 2 * cl - 1), sig), (h, oid, msg, bytes(2 * cl), sig)]
    fam["key_coord_p"] = [(h, oid, msg, min(p, ctop).to_bytes(cl, "big") + pub[cl:], sig),
                          (h, oid, msg, pub[:cl] + min(p, ctop).to_bytes(cl, "big"), sig)]
    if X + p <= ctop:
        fam["key_coord_p"].append((h, oid, msg, (X + p).to_bytes(cl, "big") + pub[cl:], sig))
    if O.CURVES[curve]["order"] != q:
        T = SF.small_order_point(curve, rng)
        fam["key_small_order"] = [(h, oid, msg, pt_bytes(curve, T), sig), (h, oid, msg, pt_bytes(curve, O.py_add(Y, T, a, p)), sig)]
    other = bytes.fromhex("0609608648016503040201")     # SHA-256's OID
    long_oid = bytes((3 * j + 1) & 0xff for j in range(64))
    fam["oid"] = [(h, other, msg, pub, sig), (h, b"", msg, pub, sig), honest(hs[0], x, pub, o=b""), honest(hs[1], x, pub, o=long_oid),
                  (h, long_oid, msg, pub, sig), honest(hs[0], x, pub, o=other)]
    fam["msg_len"] = [honest(hs[i % len(hs)], x, pub, pattern_msg(n)) for i, n in enumerate(MSG_LENS)]
    # a second key and a signature moved between keys
    x2 = rk()
    pub2 = pt_bytes(curve, fast_mul(x2, G, a, p))
    fam["other_key"] = [honest(hs[0], x2, pub2), (h, oid, msg, pub2, sig)]
    return fam


def u_zero_accepted(curve, oid, rng, hsize=32):
    """(pub, sig, digest) with u = 0 that verifies: the digest is the caller's (hash_type 0), so it can be chosen after s0.
    W = [k]G, s0 = t(W, dg) depends on dg, and u = 0 needs hbar = -s1: take s1 first, dg = LE(q - s1) (below q: hbar = dg), then
    the key x = k / v makes W' = [v]Y = W."""
    p, a, b, q, G = _curve(curve)
    ql, l = O.qlen(curve), s0_len(curve)
    if hsize < ql:
        return None
    k, s1 = 1 + rand_int(rng, q - 1), 1 + rand_int(rng, q - 1)
    dg = ((q - s1) % q).to_bytes(hsize, "little")
    W = fast_mul(k, G, a, p)
    s0 = commit_t(curve, oid, W, dg)
    v = (int.from_bytes(s0, "little") + (1 << (8 * l))) % q
    Y = fast_mul(k * pow(v, -1, q) % q, G, a, p)
    return pt_bytes(curve, Y), s0 + s1.to_bytes(ql, "little"), dg


def sign_families(curve, rng):
    """{family: [(hash name, OID, message, x, k)]}"""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    hs = hashes_for(curve)
    fam = {}

    def rmsg(n=None):
        return rng.integers(0, 256, size=int(rng.integers(1, 48)) if n is None else n, dtype=np.uint8).tobytes()

    def rx():
        return 1 + rand_int(rng, q - 1)

    fam["random"] = [(h, OID_BELT, rmsg(), rx(), rx()) for h in hs]
    m, x0, k0 = rmsg(), rx(), rx()
    fam["k_edge"] = [(hs[0], OID_BELT, m, x0, k) for k in (0, 1, q - 1, q)]
    fam["x_edge"] = [(hs[0], OID_BELT, m, x, k0) for x in (0, 1, q - 1, q)]
    fam["msg_len"] = [(hs[i % len(hs)], OID_BELT, pattern_msg(n), x0, k0) for i, n in enumerate(MSG_LENS)]
    return fam


def hbar_zero_digest(curve, hsize):
    """a digest (the caller's, hash_type 0) with hbar = 0: q itself where it fits, else zeros"""
    q = O.CURVES[curve]["q"]
    return q.to_bytes(hsize, "little") if q < (1 << (8 * hsize)) else bytes(hsize)


def random_batch(curve, n, rng, msg_len=24):
    """n items: (pubs, xs, ks, msgs) with one key per 16 items (Python's point multiplication is slow)"""
    p, a, b, q, G = _curve(curve)
    keys = [1 + rand_int(rng, q - 1) for _ in range(max(1, n // 16))]
    pubs = [pt_bytes(curve, fast_mul(x, G, a, p)) for x in keys]
    return [pubs[i % len(keys)] for i in range(n)], [keys[i % len(keys)] for i in range(n)], \
        [1 + rand_int(rng, q - 1) for _ in range(n)], [rng.integers(0, 256, size=msg_len, dtype=np.uint8).tobytes() for _ in range(n)]
