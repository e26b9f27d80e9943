"""One-call EdDSA signing two ways: the UNMODIFIED reference through ctypes on oracle/_ref/libecc_ref.so's own symbols
(eddsa_import_key_pair_from_priv_key_buf, eddsa_export_pub_key on the pair's public key, _ec_sign with adata and a NULL `rand`, the way
tests/decdsa_ref.py reaches DECDSA), and the Python restatements of tests/oracles.py (ed25519_sign / ed448_sign) behind one call.
Also the message-slot helpers and the layout of tests/golden/eddsa_sign.json."""
import ctypes as C
import hashlib
import json

import oracles as O
import sigfam_ref as R

# libecc's ec_alg_type numbers (lib_ecc_types.h:49-55) and hash_alg_type numbers
EDDSA25519, EDDSA25519CTX, EDDSA25519PH, EDDSA448, EDDSA448PH = 9, 10, 11, 12, 13
ALGS = {"EDDSA25519": 9, "EDDSA25519CTX": 10, "EDDSA25519PH": 11, "EDDSA448": 12, "EDDSA448PH": 13}
SHA512, SHAKE256 = 4, 12


def is448(alg):
    return alg >= EDDSA448


def klen(alg):
    return 57 if is448(alg) else 32


def curve_of(alg):
    return "WEI448" if is448(alg) else "WEI25519"


def is_ph(alg):
    return alg in (EDDSA25519PH, EDDSA448PH)


def takes_ctx(alg):
    return alg != EDDSA25519


def H(alg, data):
    return hashlib.shake_256(data).digest(114) if is448(alg) else hashlib.sha512(data).digest()


def PH(alg, msg):
    if not is_ph(alg):
        return msg
    return hashlib.shake_256(msg).digest(64) if is448(alg) else hashlib.sha512(msg).digest()


def dom(alg, adata):
    """dom2 / dom4 of the variant; EDDSA25519 has none"""
    if alg == EDDSA25519:
        return b""
    return (O.ed_dom4 if is448(alg) else O.ed_dom2)(1 if is_ph(alg) else 0, adata)


def expand(alg, sk):
    """(a as klen octets after the clamp of sig/eddsa.c:649-671, prefix)"""
    h = bytearray(H(alg, sk))
    kl = klen(alg)
    if is448(alg):
        h[0] &= 0xFC
        h[55] |= 0x80
        h[56] = 0
    else:
        h[0] &= 0xF8
        h[31] = (h[31] & 0x7F) | 0x40
    return bytes(h[:kl]), bytes(h[kl:])


def r_hash(alg, sk, adata, msg):
    return H(alg, dom(alg, adata) + expand(alg, sk)[1] + PH(alg, msg))


def hram(alg, adata, R_enc, A_enc, msg):
    return H(alg, dom(alg, adata) + R_enc + A_enc + PH(alg, msg))


def py_sign(alg, sk, adata, msg):
    """(public key, signature) of the restatements oracles.ed25519_sign / ed448_sign"""
    if is448(alg):
        A, sig, _ = O.ed448_sign(sk, msg, ctx=adata, prehash=is_ph(alg))
    else:
        A, sig, _ = O.ed25519_sign(sk, msg, dom=dom(alg, adata), prehash=is_ph(alg))
    return A, sig


def ref_sign(alg, sk, adata, msg):
    """(ret, public key or None, signature or None) of the reference: ret -2 where the key pair does not import, -3 where the public key
    does not export, else _ec_sign's return value.  adata None: a NULL pointer."""
    curve, kl = curve_of(alg), klen(alg)
    L, params = R.ref_params(curve)
    L.eddsa_import_key_pair_from_priv_key_buf.argtypes = [C.c_void_p, C.c_char_p, C.c_uint16, C.c_void_p, C.c_int]
    L.eddsa_init_pub_key.argtypes = [C.c_void_p, C.c_void_p]
    L.eddsa_export_pub_key.argtypes = [C.c_void_p, C.c_char_p, C.c_uint16]
    kp = C.create_string_buffer(R.BUF)
    if L.eddsa_import_key_pair_from_priv_key_buf(kp, sk, len(sk), params, alg) != 0:
        return -2, None, None
    # the pair's public key: ec_key_pair starts with its private key, from which eddsa_init_pub_key (what the import itself calls,
    # sig/eddsa.c:1042) fills a public key at an address this module knows
    pk = C.create_string_buffer(R.BUF)
    pub = C.create_string_buffer(kl)
    if L.eddsa_init_pub_key(pk, kp) != 0 or L.eddsa_export_pub_key(pk, pub, kl) != 0:
        return -3, None, None
    sig = C.create_string_buffer(2 * kl)
    mbuf = C.create_string_buffer(msg, max(1, len(msg)))       # never a NULL message (eddsa_compute_pre_hash :1058)
    ret = L._ec_sign(sig, 2 * kl, kp, mbuf, len(msg), C.cast(None, R.RAND_FN), alg, SHAKE256 if is448(alg) else SHA512,
                     adata, len(adata) if adata is not None else 0)
    return ret, pub.raw, (sig.raw if ret == 0 else None)


def load_fixture(path):
    """[item]: {"alg", "family", "sk", "adata" (hex or None), "msg", "pub", "sig" (hex or None), "ret"}"""
    with open(path) as f:
        return json.load(f)


def slot(msg, stride, length=None):
    return (len(msg) if length is None else length).to_bytes(4, "little") + msg.ljust(stride - 4, b"\0")


def stride_for(maxlen):
    return 4 + (maxlen + 3) // 4 * 4 if maxlen else 8
