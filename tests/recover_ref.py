"""ECDSA public-key recovery by the UNMODIFIED reference, and the crafted inputs of the recovery tests.

oracle/ref_driver.c has no recovery entry; none is needed: oracle/_ref/libecc_ref.so exports the reference's own symbols, and
ctypes can call them on opaque, oversized buffers (an ec_params in 64 KB, an ec_pub_key in 8 KB):
    ec_get_curve_params_by_name, import_params, ecdsa_public_key_from_sig, ec_pub_key_export_to_buf, ec_pub_key_export_to_aff_buf.
The reference's answer for one item is (ret, key1, key2): ret 0 / -1, each key its affine X || Y bytes, or the point at
infinity (which ec_pub_key_export_to_aff_buf has no bytes for)."""
import ctypes as C
import threading

import numpy as np

import oracles as O

ECAMD_OK, ECAMD_ERR, ECAMD_INF = 0, 1, 2
# the curves of the recovery fixture: a = -3, a = 0, two larger fields, a generic a, q > p with qlen != clen, cofactor 8
CURVES = ["SECP256R1", "SECP256K1", "SECP384R1", "SECP521R1", "BRAINPOOLP256R1", "SECP224K1", "WEI25519"]
PRIME_ORDER = [c for c in CURVES if c != "WEI25519"]
FAMILIES = ["honest", "not_abscissa", "range", "e_zero", "digest_len", "redo"]   # + "r_geq_p" where q > p
PARAMS_BYTES, KEY_BYTES = 1 << 16, 1 << 13

_lock = threading.Lock()
_params = {}


def _lib():
    L = C.CDLL(O.REF_SO)
    L.ec_get_curve_params_by_name.argtypes = [C.c_char_p, C.c_uint8, C.POINTER(C.c_void_p)]
    L.import_params.argtypes = [C.c_void_p, C.c_void_p]
    L.ecdsa_public_key_from_sig.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint8, C.c_char_p, C.c_uint8]
    L.ec_pub_key_export_to_aff_buf.argtypes = [C.c_void_p, C.c_char_p, C.c_uint8]
    L.ec_pub_key_export_to_buf.argtypes = [C.c_void_p, C.c_char_p, C.c_uint8]
    return L


def ref_params(curve):
    """(library, imported ec_params buffer) of a curve, made once and then only read"""
    with _lock:
        if curve not in _params:
            L = _lib()
            name = curve.encode() + b"\0"
            sp = C.c_void_p()
            assert L.ec_get_curve_params_by_name(name, len(name), C.byref(sp)) == 0 and sp.value, curve
            buf = C.create_string_buffer(PARAMS_BYTES)
            assert L.import_params(buf, sp) == 0
            _params[curve] = (L, buf)
        return _params[curve]


def ref_recover(curve, sigs, digests, hlen):
    """the reference item by item: (pub1, pub2, status1, status2) in the layout of ec_ecdsa_recover_batch"""
    L, params = ref_params(curve)
    cl, ql = O.clen(curve), O.qlen(curve)
    n = len(sigs) // (2 * ql)
    assert len(sigs) == n * 2 * ql and len(digests) == n * hlen
    k1, k2 = C.create_string_buffer(KEY_BYTES), C.create_string_buffer(KEY_BYTES)
    out, prj = C.create_string_buffer(2 * cl), C.create_string_buffer(3 * cl)
    zero = bytes(2 * cl)
    p1, p2, s1, s2 = [], [], bytearray(n), bytearray(n)

    def export(key):
        # the projective export (X || Y || Z) takes every key the function returns; Z = 0 is the point at infinity, which has no affine form
        assert L.ec_pub_key_export_to_buf(key, prj, 3 * cl) == 0
        if prj.raw[2 * cl:3 * cl] == bytes(cl):
            return zero, ECAMD_INF
        assert L.ec_pub_key_export_to_aff_buf(key, out, 2 * cl) == 0
        return out.raw[:2 * cl], ECAMD_OK

    for i in range(n):
        C.memset(k1, 0, KEY_BYTES)
        C.memset(k2, 0, KEY_BYTES)
        ret = L.ecdsa_public_key_from_sig(k1, k2, params, sigs[2 * ql * i:2 * ql * (i + 1)], 2 * ql,
                                          digests[hlen * i:hlen * (i + 1)], hlen)
        if ret != 0:
            p1.append(zero)
            p2.append(zero)
            s1[i] = s2[i] = ECAMD_ERR
            continue
        a, s1[i] = export(k1)
        b, s2[i] = export(k2)
        p1.append(a)
        p2.append(b)
    return b"".join(p1), b"".join(p2), bytes(s1), bytes(s2)


def ref_recover_threaded(curve, sigs, digests, hlen):
    ql = O.qlen(curve)
    n = len(sigs) // (2 * ql)
    ref_params(curve)
    parts = O.in_slices(lambda lo, hi: ref_recover(curve, sigs[2 * ql * lo:2 * ql * hi], digests[hlen * lo:hlen * hi], hlen), n)
    return O.join_slices(parts)


# ---- inputs, with Python integers ----
def _curve(curve):
    c = O.CURVES[curve]
    return c["p"], c["a"], c["b"], c["q"], (c["gx"], c["gy"])


def digest_to_e(dg, q):
    e = int.from_bytes(dg, "big")
    qbits = q.bit_length()
    if 8 * len(dg) > qbits:
        e >>= 8 * len(dg) - qbits
    return e % q


def sign(curve, x, k, dg):
    """(r, s) of the ECDSA signature with private key x and nonce k, or None where the signer would restart"""
    p, a, b, q, G = _curve(curve)
    R = O.py_mul(k, G, a, p)
    r = R[0] % q
    s = pow(k, -1, q) * (digest_to_e(dg, q) + x * r) % q
    return (r, s) if r and s else None


def sig_bytes(curve, r, s):
    ql = O.qlen(curve)
    return r.to_bytes(ql, "big") + s.to_bytes(ql, "big")


def rand_int(rng, below):
    nb = (below.bit_length() + 7) // 8 + 8
    return int.from_bytes(rng.integers(0, 256, size=nb, dtype=np.uint8).tobytes(), "big") % below


def pub_bytes(curve, x):
    p, a, b, q, G = _curve(curve)
    cl = O.clen(curve)
    Y = O.py_mul(x, G, a, p)
    return Y[0].to_bytes(cl, "big") + Y[1].to_bytes(cl, "big")


def is_abscissa(curve, x):
    p, a, b, q, G = _curve(curve)
    if x >= p:
        return False
    w = (x * x * x + a * x + b) % p
    return w == 0 or pow(w, (p - 1) // 2, p) == 1


def crafted_families(curve, rng):
    """{family: [(sig bytes, digest bytes, signer's key bytes or None)]}: the families of tests/golden/ecdsa_recover.json"""
    p, a, b, q, G = _curve(curve)
    ql = O.qlen(curve)
    fam = {}

    def rdigest(n=32):
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()

    def honest(dg):
        while True:
            x, k = 1 + rand_int(rng, q - 1), 1 + rand_int(rng, q - 1)
            rs = sign(curve, x, k, dg)
            if rs:
                return sig_bytes(curve, *rs), dg, pub_bytes(curve, x)

    fam["honest"] = [honest(rdigest()) for _ in range(16)]
    items = []
    while len(items) < 6:
        r = 1 + rand_int(rng, min(p, q) - 1)
        if not is_abscissa(curve, r):
            items.append((sig_bytes(curve, r, 1 + rand_int(rng, q - 1)), rdigest(), None))
    fam["not_abscissa"] = items
    hs, hd, _ = honest(rdigest())
    r0, s0 = int.from_bytes(hs[:ql], "big"), int.from_bytes(hs[ql:], "big")
    top = (1 << (8 * ql)) - 1
    fam["range"] = [(sig_bytes(curve, r, s), hd, None) for r, s in
                    [(0, s0), (r0, 0), (q, s0), (r0, q), (q - 1, s0), (r0, q - 1), (min(top, q + 1), s0), (top, s0), (r0, top)]]
    if q > p:
        fam["r_geq_p"] = [(sig_bytes(curve, r, s0), hd, None) for r in (p, p + 1, q - 2, (p + q) // 2)]
    # e = 0 mod q: zero digests, and the digest q itself (e = 0 where 8 qlen = |q|; where it is longer the shift makes it q >> k)
    fam["e_zero"] = [honest(dg)[:2] + (None,) for dg in (bytes(32), bytes(ql), q.to_bytes(ql, "big"), bytes(64))]
    fam["digest_len"] = [honest(rdigest(n)) for n in (20, 32, 48, 64) for _ in range(2)]
    # s = +-e / k with r = x([k]G): [v]R = +-[e / r]G = -+[u]G, so one candidate is the point at infinity and the other a doubling
    items = []
    while len(items) < 6:
        k, dg = 1 + rand_int(rng, q - 1), rdigest()
        e = digest_to_e(dg, q)
        r = O.py_mul(k, G, a, p)[0]
        if e == 0 or r == 0 or r >= q:
            continue
        for sgn in (1, -1):
            items.append((sig_bytes(curve, r, sgn * e * pow(k, -1, q) % q), dg, None))
    fam["redo"] = items
    return fam


def random_batch(curve, n, rng, sign_batch):
    """n items, the first half honest (signed by sign_batch(privs, nonces, digests) -> (sigs, status)), the second half with
    random r and s in [1, q - 1]: (sigs, digests, private keys of the honest half)"""
    p, a, b, q, G = _curve(curve)
    ql = O.qlen(curve)
    nh = n // 2

    def scalars(m):
        raw = rng.integers(0, 256, size=(m, ql + 8), dtype=np.uint8)
        return b"".join((1 + int.from_bytes(row.tobytes(), "big") % (q - 1)).to_bytes(ql, "big") for row in raw)

    digests = rng.integers(0, 256, size=32 * n, dtype=np.uint8).tobytes()
    privs, nonces = scalars(nh), scalars(nh)
    sigs, st = sign_batch(privs, nonces, digests[:32 * nh])
    assert st == bytes(nh), "the signer restarted on a random nonce"
    rnd_r, rnd_s = scalars(n - nh), scalars(n - nh)
    tail = b"".join(rnd_r[ql * i:ql * (i + 1)] + rnd_s[ql * i:ql * (i + 1)] for i in range(n - nh))
    return sigs + tail, digests, privs
