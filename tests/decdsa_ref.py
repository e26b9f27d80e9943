"""Deterministic ECDSA (RFC 6979) two ways: the UNMODIFIED reference through ctypes on oracle/_ref/libecc_ref.so's own symbols
(ec_key_pair_import_from_priv_key_buf + _ec_sign with DECDSA and no `rand` hook, the way tests/sigfam_ref.py reaches it), and a
Python restatement of the reference's generator (__ecdsa_rfc6979_nonce, sig/ecdsa_common.c:48-169) that also counts the rejected
candidates -- oracles.rfc6979_nonce is the same generator without the counter (and with RFC 6979's `1 <= k`, which the reference
leaves to the signing step; no item here has k = 0)."""
import ctypes as C
import hashlib
import hmac
import json

import oracles as O
import sigfam_ref as R
from bign_ref import fast_mul

DECDSA = 14                                      # libecc's ec_alg_type number
CURVES = ["SECP192R1", "SECP224K1", "SECP256R1", "SECP256K1", "BRAINPOOLP256R1", "BRAINPOOLP384R1", "SECP521R1"]
RETRY_CURVES = ["SECP224K1", "BRAINPOOLP256R1", "BRAINPOOLP384R1"]   # the orders far enough below 2^qbits to reject candidates
HASHES = ["SHA224", "SHA256", "SHA384", "SHA512"]
HT = {"SHA224": 1, "SHA256": 2, "SHA384": 3, "SHA512": 4}
HSIZE = {"SHA224": 28, "SHA256": 32, "SHA384": 48, "SHA512": 64}
MSG_LENS = [0, 1, 55, 56, 64, 111, 112, 200]
MAX_RETRIES = 1000


def H(hash_name, data):
    return hashlib.new(O.HASHLIB[hash_name], data).digest()


def nonce_from_digest(curve, hash_name, priv, h1):
    """(k, rejected candidates) from the key's qlen octets and the digest; (0, MAX_RETRIES) when the bound is reached"""
    q = O.CURVES[curve]["q"]
    qbits, rlen = q.bit_length(), (q.bit_length() + 7) // 8
    hname = O.HASHLIB[hash_name]
    hl = len(h1)
    assert len(priv) == rlen and hl == HSIZE[hash_name]

    def bits2int(b):
        x = int.from_bytes(b, "big")
        return x >> (len(b) * 8 - qbits) if len(b) * 8 > qbits else x

    bx = priv + (bits2int(h1) % q).to_bytes(rlen, "big")
    V, K = b"\x01" * hl, b"\x00" * hl
    K = hmac.new(K, V + b"\x00" + bx, hname).digest()
    V = hmac.new(K, V, hname).digest()
    K = hmac.new(K, V + b"\x01" + bx, hname).digest()
    V = hmac.new(K, V, hname).digest()
    retries = 0
    while True:
        T = b""
        while 8 * len(T) < qbits:
            V = hmac.new(K, V, hname).digest()
            T += V
        k = bits2int(T[:rlen])
        if k < q:
            return k, retries
        retries += 1
        if retries >= MAX_RETRIES:
            return 0, retries
        K = hmac.new(K, V + b"\x00", hname).digest()
        V = hmac.new(K, V, hname).digest()


def nonce(curve, hash_name, priv, msg):
    return nonce_from_digest(curve, hash_name, priv, H(hash_name, msg))


def sign_with(curve, x, k, h1):
    """(status, r || s) of ec_ecdsa_sign_batch's rules in Python integers: x < q, k in [1, q - 1], r, s != 0, e != x r"""
    c = O.CURVES[curve]
    q, ql = c["q"], O.qlen(curve)
    bad = (1, bytes(2 * ql))
    if x >= q or not 0 < k < q:
        return bad
    W = fast_mul(k, (c["gx"], c["gy"]), c["a"], c["p"])
    r = W[0] % q
    e = int.from_bytes(h1, "big")
    if 8 * len(h1) > q.bit_length():
        e >>= 8 * len(h1) - q.bit_length()
    e %= q
    if r == 0 or e == x * r % q:
        return bad
    s = pow(k, -1, q) * (x * r + e) % q
    if s == 0:
        return bad
    return 0, r.to_bytes(ql, "big") + s.to_bytes(ql, "big")


def ref_sign(curve, hash_name, priv, msg):
    """(ret, signature or None) of the reference: ret -2 where ec_key_pair_import_from_priv_key_buf fails, -1 where _ec_sign does"""
    L, params = R.ref_params(curve)
    ql = O.qlen(curve)
    kp = C.create_string_buffer(R.BUF)
    if L.ec_key_pair_import_from_priv_key_buf(kp, params, priv, len(priv), DECDSA) != 0:
        return -2, None
    sig = C.create_string_buffer(2 * ql)
    ret = L._ec_sign(sig, 2 * ql, kp, msg, len(msg), C.cast(None, R.RAND_FN), DECDSA, O.HASH_IDS[hash_name], None, 0)
    return (0, sig.raw[:2 * ql]) if ret == 0 else (-1, None)


def load_fixture(path):
    """{curve: [item]}: item = {"hash", "msg", "x" (qlen octets, hex), "ret", "sig" (hex or None), "k" (hex), "retries", "family"}"""
    with open(path) as f:
        return json.load(f)


def slot(msg, stride, length=None):
    return (len(msg) if length is None else length).to_bytes(4, "little") + msg.ljust(stride - 4, b"\0")


def stride_for(maxlen):
    return 4 + (maxlen + 3) // 4 * 4 if maxlen else 8
