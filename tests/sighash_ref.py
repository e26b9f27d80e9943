"""ECSDSA, ECOSDSA and ECKCDSA three ways: a Python-integer restatement of the sign and verify rules, the UNMODIFIED reference
through ctypes (the symbols tests/sigfam_ref.py already reaches in oracle/_ref/libecc_ref.so), and the crafted inputs of the
tests.

The reference hashes the message itself, so an item is (message, hash name).  What the GPU entry points take is built here:
for ECSDSA / ECOSDSA a slot `u32 length | blank | message` (the blank is where the device writes the commitment), for ECKCDSA
the digest h = H(z || m) with z the first block-size octets of Yx || Yy, zero padded."""
import ctypes as C
import hashlib

import numpy as np

import oracles as O
import sigfam_ref as SF

ECKCDSA, ECSDSA, ECOSDSA = 2, 3, 4                 # libecc's ec_alg_type numbers
SCHEMES = {"ECKCDSA": ECKCDSA, "ECSDSA": ECSDSA, "ECOSDSA": ECOSDSA}
CURVES = SF.CURVES
HSIZE = {"SHA224": 28, "SHA256": 32, "SHA384": 48, "SHA512": 64}
BLOCK = {"SHA224": 64, "SHA256": 64, "SHA384": 128, "SHA512": 128}
PAD_EDGES = (0, 1, 55, 56, 63, 64, 111, 112, 119, 120)    # message lengths beyond the blank around SHA-2's padding boundaries

H = SF.H
rand_int = SF.rand_int
pt_bytes = SF.pt_bytes
import_pub = SF.import_pub
_curve = SF._curve


def hashes_for(curve):
    """every truncation case: hsize < qlen (SHA-224 / SHA-256 on the large curves), = qlen, > qlen with an ECKCDSA shift of
    3 (SHA-256 on SECP224K1: qlen 29), 32 (SHA-512, 256-bit) and 16 (SHA-512 on SECP384R1)"""
    if curve == "SECP521R1":
        return ["SHA224", "SHA256", "SHA512"]
    if curve == "SECP384R1":
        return ["SHA256", "SHA512", "SHA384"]
    return ["SHA256", "SHA512"]


def r_len(alg, hash_name, ql):
    return min(HSIZE[hash_name], ql) if alg == ECKCDSA else HSIZE[hash_name]


def blank_len(alg, cl):
    return 2 * cl if alg == ECSDSA else cl


def pub_point(curve, alg, x):
    """[1/x]G for ECKCDSA, [x]G for the others"""
    p, a, b, q, G = _curve(curve)
    return O.py_mul(pow(x, -1, q) if alg == ECKCDSA else x, G, a, p)


def kcdsa_h(curve, hash_name, pub, msg):
    """ECKCDSA's h = H(z || m)"""
    return H(hash_name, (pub + bytes(BLOCK[hash_name]))[:BLOCK[hash_name]] + msg)


def slot(alg, cl, msg, stride, length=None):
    """a message slot with the blank left empty; length: the length word, when it is not the honest one"""
    bl = blank_len(alg, cl)
    body = bytes(bl) + msg
    ln = len(body) if length is None else length
    assert 4 + len(body) <= stride
    return ln.to_bytes(4, "little") + body + bytes(stride - 4 - len(body))


def stride_for(alg, cl, max_msg):
    return (4 + blank_len(alg, cl) + max_msg + 3) & ~3


def device_input(curve, alg, hash_name, pub, msg, stride=None):
    """what ec_sig_hashed_* takes for this item: the slot (stride given) or ECKCDSA's digest"""
    if alg == ECKCDSA:
        return kcdsa_h(curve, hash_name, pub, msg)
    return slot(alg, O.clen(curve), msg, stride)


# ---------------------------------------------------------------------------------------------------------------------
# the Python-integer restatement
# ---------------------------------------------------------------------------------------------------------------------
def commit_hash(curve, alg, hash_name, W, msg):
    cl = O.clen(curve)
    if alg == ECKCDSA:
        return H(hash_name, W[0].to_bytes(cl, "big"))
    return H(hash_name, W[0].to_bytes(cl, "big") + (W[1].to_bytes(cl, "big") if alg == ECSDSA else b"") + msg)


def kcdsa_e(r, h, q):
    return int.from_bytes(bytes(x ^ y for x, y in zip(r, h[len(h) - len(r):])), "big") % q


def front_end(curve, alg, hash_name, pub, sig, msg):
    """(flag, u of G, v of Y)"""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    rl = r_len(alg, hash_name, ql)
    r, s = sig[:rl], int.from_bytes(sig[rl:], "big")
    if not 0 < s < q:
        return 1, 0, 0
    if alg == ECKCDSA:
        return 0, kcdsa_e(r, kcdsa_h(curve, hash_name, pub, msg), q), s
    e = -int.from_bytes(r, "big") % q
    if e == 0:
        return 1, 0, 0
    return 0, s, e


def verify(curve, alg, hash_name, pub, sig, msg):
    """0 accept / 1 reject"""
    p, a, b, q, G = _curve(curve)
    rl = r_len(alg, hash_name, O.qlen(curve))
    Y = import_pub(curve, pub)
    if Y is None:
        return 1
    flag, u, v = front_end(curve, alg, hash_name, pub, sig, msg)
    if flag:
        return 1
    W = O.py_add(O.py_mul(u, G, a, p), O.py_mul(v, Y, a, p), a, p)
    if W is None:
        return 1
    return 0 if commit_hash(curve, alg, hash_name, W, msg)[HSIZE[hash_name] - rl:] == sig[:rl] else 1


def key_ok(alg, q, x):
    """what the recording shows: ECKCDSA's key pair imports for 0 < x < q only; ECSDSA and ECOSDSA sign with any x of qlen
    bytes, 0 and values >= q included (no range check in sig/ecsdsa_common.c)"""
    return 0 < x < q if alg == ECKCDSA else True


def sign(curve, alg, hash_name, x, k, msg):
    """(status, signature bytes) as ec_sig_hashed_sign_batch returns them"""
    p, a, b, q, G = _curve(curve)
    ql = O.qlen(curve)
    rl = r_len(alg, hash_name, ql)
    bad = (1, bytes(rl + ql))
    if not key_ok(alg, q, x) or not 0 < k < q:
        return bad
    W = O.py_mul(k, G, a, p)
    dg = commit_hash(curve, alg, hash_name, W, msg)
    r = dg[len(dg) - rl:]
    if alg == ECKCDSA:
        pub = pt_bytes(curve, pub_point(curve, alg, x))
        s = x * (k - kcdsa_e(r, kcdsa_h(curve, hash_name, pub, msg), q)) % q
    else:
        e = int.from_bytes(r, "big") % q
        if e == 0:
            return bad
        s = (k + e * x) % q
    if s == 0:
        return bad
    return 0, r + s.to_bytes(ql, "big")


# ---------------------------------------------------------------------------------------------------------------------
# the reference through ctypes
# ---------------------------------------------------------------------------------------------------------------------
def ref_verify(curve, alg, hash_name, pub, sig, msg):
    """ec_pub_key_import_from_aff_buf + ec_verify: 0 / -1"""
    L, params = SF.ref_params(curve)
    key = C.create_string_buffer(SF.BUF)
    if L.ec_pub_key_import_from_aff_buf(key, params, pub, len(pub), alg) != 0:
        return -1
    return -1 if L.ec_verify(sig, len(sig), key, msg, len(msg), alg, O.HASH_IDS[hash_name], None, 0) != 0 else 0


def ref_sign(curve, alg, hash_name, x, k, msg):
    """ec_key_pair_import_from_priv_key_buf + _ec_sign with the nonce k: (ret, signature bytes or None); ret -2: the key pair
    import failed.  The nonce hook fails for k >= q and on a second call (a restart), as in sigfam_ref.ref_sign."""
    L, params = SF.ref_params(curve)
    ql = O.qlen(curve)
    sl = r_len(alg, hash_name, ql) + ql
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
    ret = L._ec_sign(sig, sl, kp, msg, len(msg), cb, alg, O.HASH_IDS[hash_name], None, 0)
    return (0, sig.raw[:sl]) if ret == 0 else (-1, None)


# fields the fixture file leaves out where the previous item has the same; a signature is filed as its halves "r" and "s"
DELTA = ("family", "hash", "msg", "pub", "r", "s", "x", "k")


def pattern_msg(n):
    """the long message of the fixture, which the file names by its length alone ("msgpat")"""
    return bytes((7 * j + 3) & 0xff for j in range(n))


def load_fixture(path):
    """tests/golden/sig_hashed.json with the left-out fields put back"""
    import json
    with open(path) as f:
        fx = json.load(f)
    for per in fx.values():
        for d in per.values():
            for items in d.values():
                for j, i in enumerate(items):
                    if "msgpat" in i:
                        i["msg"] = pattern_msg(i.pop("msgpat")).hex()
                    for k in DELTA:
                        if j and k not in i and k in items[j - 1]:
                            i[k] = items[j - 1][k]
                    if "r" in i:
                        i["sig"] = i["r"] + i["s"]
    return fx


# ---------------------------------------------------------------------------------------------------------------------
# crafted inputs
# ---------------------------------------------------------------------------------------------------------------------
def verify_families(curve, alg, rng):
    """{family: [(hash name, message, public key bytes, signature bytes)]}"""
    p, a, b, q, G = _curve(curve)
    ql, cl = O.qlen(curve), O.clen(curve)
    hs = hashes_for(curve)
    fam = {}

    def rmsg(n=None):
        return rng.integers(0, 256, size=int(rng.integers(1, 48)) if n is None else n, dtype=np.uint8).tobytes()

    def keypair():
        x = 1 + rand_int(rng, q - 1)
        return x, pt_bytes(curve, pub_point(curve, alg, x))

    def honest(h, x, pub, msg=None):
        while True:
            m = rmsg() if msg is None else msg
            st, sig = sign(curve, alg, h, x, 1 + rand_int(rng, q - 1), m)
            if st == 0:
                return h, m, pub, sig

    def sb(h, r, s):
        return r + s.to_bytes(ql, "big")

    x, pub = keypair()
    fam["honest"] = [honest(h, x, pub) for h in hs]
    h, msg, pub, sig = honest(hs[0], x, pub)
    rl = r_len(alg, h, ql)
    r0, s0 = sig[:rl], int.from_bytes(sig[rl:], "big")

    def flip(bs, i):
        return bs[:i] + bytes([bs[i] ^ 1]) + bs[i + 1:]

    fam["tampered"] = [(h, msg, pub, flip(sig, 0)), (h, msg, pub, flip(sig, rl - 1)), (h, msg, pub, flip(sig, rl)),
                       (h, msg, pub, flip(sig, rl + ql - 1)), (h, flip(msg, 0), pub, sig), (h, msg + b"!", pub, sig),
                       (h, msg, keypair()[1], sig)]
    top = (1 << (8 * ql)) - 1
    fam["s_range"] = [(h, msg, pub, sb(h, r0, s)) for s in (0, q - 1, q, min(top, q + 1), top)]
    # OS2I(r) = 0 mod q: rejected by ECSDSA / ECOSDSA (e = 0); for ECKCDSA just another r
    for hh in hs:
        hz = HSIZE[hh]
        rlh = r_len(alg, hh, ql)
        vals = [0, q, 2 * q] if alg != ECKCDSA else [0]
        fam.setdefault("r_zero_mod_q", []).extend(
            (hh, msg, pub, v.to_bytes(rlh, "big") + s0.to_bytes(ql, "big")) for v in vals if v < (1 << (8 * rlh)))
    if alg == ECKCDSA:
        # r = h' (e = 0, allowed): W' = [s]Y alone, a summand at infinity.  Through the reference, which hashes z || m itself, such
        # an item cannot be made to verify without inverting the hash, so these are rejected ones; the accepted e = 0 item is
        # built at the level of the entry point, which takes h from the caller (kcdsa_e_zero_accepted).
        for hh in hs:
            m2 = rmsg()
            hp = kcdsa_h(curve, hh, pub, m2)
            rlh = r_len(alg, hh, ql)
            fam.setdefault("e_zero", []).append((hh, m2, pub, hp[len(hp) - rlh:] + (1 + rand_int(rng, q - 1)).to_bytes(ql, "big")))
    # W' at infinity and a doubling: [u]G = -[v]Y and [u]G = [v]Y, with s chosen after e (the hash then decides: rejected)
    winf, equal = [], []
    for hh in hs:
        m2 = rmsg()
        rlh = r_len(alg, hh, ql)
        r = rng.integers(0, 256, size=rlh, dtype=np.uint8).tobytes()
        if alg == ECKCDSA:
            e = kcdsa_e(r, kcdsa_h(curve, hh, pub, m2), q)            # W' = [s / x]G + [e]G
            s_inf, s_eq = -e * x % q, e * x % q
        else:
            e = -int.from_bytes(r, "big") % q                          # W' = [s]G + [e x]G
            s_inf, s_eq = -e * x % q, e * x % q
        if s_inf:
            winf.append((hh, m2, pub, r + s_inf.to_bytes(ql, "big")))
        if s_eq:
            equal.append((hh, m2, pub, r + s_eq.to_bytes(ql, "big")))
    fam["w_infinity"] = winf
    fam["equal_operands"] = equal
    # keys that do not import: a coordinate >= p, a point off the curve, (0, 0)
    X, Y = int.from_bytes(pub[:cl], "big"), int.from_bytes(pub[cl:], "big")
    ctop = (1 << (8 * cl)) - 1
    bad = [bytes(2 * cl), flip(pub, 0), flip(pub, 2 * cl - 1)]
    bad.append((X + p if X + p <= ctop else min(p, ctop)).to_bytes(cl, "big") + pub[cl:])
    bad.append(pub[:cl] + (Y + p if Y + p <= ctop else min(p, ctop)).to_bytes(cl, "big"))
    fam["key_not_importable"] = [(h, msg, k, sig) for k in bad]
    if O.CURVES[curve]["order"] != q:
        T = SF.small_order_point(curve, rng)
        fam["key_small_order"] = [(h, msg, pt_bytes(curve, T), sig)]
        fam["key_torsion"] = [(h, msg, pt_bytes(curve, O.py_add((X, Y), T, a, p)), sig)]
    # SHA padding boundaries: message lengths beyond the blank (ECKCDSA hashes no message on the device: its h covers them)
    fam["pad_edges"] = [honest(hs[i % len(hs)], x, pub, pattern_msg(n)) for i, n in enumerate(PAD_EDGES if alg != ECKCDSA else (0, 64))]
    fam["longest"] = [honest(hs[0], x, pub, pattern_msg(4096 - 4 - blank_len(alg, cl)))]
    # signatures of the ECDSA-shaped schemes are no signatures here (r_len = qlen only where the sizes agree: padded or cut to fit)
    dg = H(hs[0], msg)
    for other in (SF.ECGDSA,):
        st, osig = SF.sign(curve, other, x, 1 + rand_int(rng, q - 1), dg)
        rl0 = r_len(alg, hs[0], ql)
        fam["foreign_scheme"] = [(hs[0], msg, pub, osig[:ql].rjust(rl0, b"\0")[-rl0:] + osig[ql:])]
    return fam


def kcdsa_e_zero_accepted(curve, hash_name, rng):
    """(pub, sig, h) with r = h': an ECKCDSA item that is honest for e = 0 -- r from [k]G, h chosen to end in r, s = x k"""
    p, a, b, q, G = _curve(curve)
    ql = O.qlen(curve)
    rl = r_len(ECKCDSA, hash_name, ql)
    x, k = 1 + rand_int(rng, q - 1), 1 + rand_int(rng, q - 1)
    dg = commit_hash(curve, ECKCDSA, hash_name, O.py_mul(k, G, a, p), b"")
    r = dg[len(dg) - rl:]
    h = rng.integers(0, 256, size=HSIZE[hash_name] - rl, dtype=np.uint8).tobytes() + r
    return pt_bytes(curve, pub_point(curve, ECKCDSA, x)), r + (x * k % q).to_bytes(ql, "big"), h


def sign_families(curve, alg, rng):
    """{family: [(hash name, message, x, k)]}"""
    q = O.CURVES[curve]["q"]
    ql = O.qlen(curve)
    hs = hashes_for(curve)
    top = (1 << (8 * ql)) - 1
    fam = {}

    def rmsg(n=None):
        return rng.integers(0, 256, size=int(rng.integers(1, 48)) if n is None else n, dtype=np.uint8).tobytes()

    def rx():
        return 1 + rand_int(rng, q - 1)

    fam["honest"] = [(h, rmsg(), rx(), rx()) for h in hs]
    m, x0, k0 = rmsg(), rx(), rx()
    fam["x_edge"] = [(hs[0], m, x, k0) for x in (0, q - 1, q, min(top, q + 1), top)]
    fam["k_edge"] = [(hs[0], m, x0, k) for k in (0, q - 1, q, min(top, q + 1))]
    # (every length of PAD_EDGES is recorded on the verification side, whose items the reference's signer made; the GPU tests sign
    # them all and check against the reference at run time)
    fam["pad_edges"] = [(hs[i % len(hs)], pattern_msg(n), x0, k0) for i, n in enumerate((0, 64))]
    return fam


def random_batch(curve, alg, hash_name, n, rng, msg_len=24):
    """n items: (pubs, privs, nonces, msgs) with one key per 16 items (Python's point multiplication is slow)"""
    q = O.CURVES[curve]["q"]
    keys = [1 + rand_int(rng, q - 1) for _ in range(max(1, n // 16))]
    pubs = [pt_bytes(curve, pub_point(curve, alg, x)) for x in keys]
    xs = [keys[i % len(keys)] for i in range(n)]
    return [pubs[i % len(keys)] for i in range(n)], xs, [1 + rand_int(rng, q - 1) for _ in range(n)], \
        [rng.integers(0, 256, size=msg_len, dtype=np.uint8).tobytes() for _ in range(n)]
