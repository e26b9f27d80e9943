"""DBIGN's and BIP0340's nonce generators two ways: Python restatements of the reference's __bign_determinitic_nonce
(sig/bign_common.c:200-342, with a count of the rejected candidates) and of _bip0340_sign's derivation (sig/bip0340.c:213-294,
through schnorr_ref.bip0340_nonce), and the UNMODIFIED reference through ctypes on oracle/_ref/libecc_ref.so's own symbols
(ec_key_pair_import_from_priv_key_buf + _ec_sign: DBIGN with libecc's adata framing of OID and t, BIP0340 with the aux value from the
`rand` hook).  The signatures from a nonce are bign_ref.sign_digest's and schnorr_ref.sign's; the slots are theirs too."""
import ctypes as C
import json

import oracles as O
import sigfam_ref as SF
import bign_ref as B
import schnorr_ref as S

DBIGN_CURVES = ["BIGN256V1", "BIGN384V1", "BIGN512V1", "SECP521R1", "SECP224K1", "WEI25519"]
DBIGN_HASHES = ["BELT", "SHA224", "SHA256", "SHA384", "SHA512"]
RETRY_CURVES = ["SECP224K1", "WEI25519"]           # the orders that reject about half of the candidates (15 in 16 on two blocks of WEI25519)
BIP_CURVES = ["SECP256K1", "SECP256R1", "SECP384R1", "SECP521R1", "WEI25519"]
BIP_HASHES = ["SHA224", "SHA256", "SHA384", "SHA512"]
HSIZE = dict(B.HSIZE, SHA384=48)
HT = dict(S.HASH_TYPE, BELT=B.HASH_BELT)
MAX_REJECTS = 1000
T_SAMPLE = bytes.fromhex("BE32971343FC9A48A02A885F194B09A17ECDA4D01544AF")   # the additional data of the standard's own example


def H(hash_name, data):
    return B.H(hash_name, data)


def blocks(hlen):
    return max(2, hlen // 16)


def dbign_nonce_from_digest(curve, priv, dg, oid, t):
    """(status, k, candidates rejected at i >= 2 n) from the key's qlen octets and the digest; (1, 0, MAX_REJECTS) at the cap"""
    q = O.CURVES[curve]["q"]
    qbits, ql = q.bit_length(), O.qlen(curve)
    assert len(priv) == ql and 1 <= len(dg) <= 128
    l = ql // 2
    theta = B.belt_hash(oid + priv[::-1][:2 * l] + t)
    n = blocks(len(dg))
    r = bytearray(dg.ljust(16 * 8, b"\0"))
    i, rej = 1, 0
    while True:
        s = bytes(16)
        for j in range(n - 1):
            s = B._xor(s, r[16 * j:16 * j + 16])
        r[0:16 * (n - 2)] = r[16:16 * (n - 1)]
        new = B._xor(B._xor(B.belt_encrypt(s, theta), r[16 * (n - 1):16 * n]), i.to_bytes(4, "little") + bytes(12))
        r[16 * (n - 2):16 * (n - 1)] = new
        r[16 * (n - 1):16 * n] = s
        if ql < 16 * n:
            k = int.from_bytes(r[:ql], "little") & ((1 << qbits) - 1)
        else:
            k = int.from_bytes(r[:16 * n], "little")
        if i >= 2 * n:
            if 0 < k < q:
                return 0, k, rej
            rej += 1
            if rej >= MAX_REJECTS:
                return 1, 0, rej
        i += 1


def dbign_nonce(curve, hash_name, x, oid, t, msg):
    return dbign_nonce_from_digest(curve, (x % (1 << (8 * O.qlen(curve)))).to_bytes(O.qlen(curve), "big"), H(hash_name, msg), oid, t)


def dbign_sign(curve, hash_name, x, oid, t, msg):
    """(status, signature bytes) as ec_dbign_sign_batch returns them, and the restatement's (k, rejected)"""
    st, k, rej = dbign_nonce(curve, hash_name, x, oid, t, msg)
    return B.sign_digest(curve, oid, x, k, H(hash_name, msg)), (k, rej)


def ref_dbign_sign(curve, hash_name, oid, t, x, msg):
    """ec_key_pair_import_from_priv_key_buf + _ec_sign(DBIGN) with no `rand` hook: (ret, signature or None); ret -2: the import failed"""
    L, params = SF.ref_params(curve)
    ql, sl = O.qlen(curve), B.sig_len(curve)
    kp = C.create_string_buffer(SF.BUF)
    if L.ec_key_pair_import_from_priv_key_buf(kp, params, x.to_bytes(ql, "big"), ql, B.DBIGN) != 0:
        return -2, None
    sig = C.create_string_buffer(sl)
    ad = B.adata(oid, t)
    ret = L._ec_sign(sig, sl, kp, msg, len(msg), C.cast(None, SF.RAND_FN), B.DBIGN, B.HASH_IDS[hash_name], ad, len(ad))
    return (0, sig.raw[:sl]) if ret == 0 else (-1, None)


def bip_pub(curve, x):
    """[x]G as affine bytes, or None"""
    p, a, b, q, G = S._curve(curve)
    Y = S.py_mul(x % q, G, a, p) if x % q else None
    return None if Y is None else S.pt_bytes(curve, Y)


def bip_nonce(curve, hash_name, x, aux, msg, pub=None):
    """(status, k) of ec_bip0340_nonce_batch; pub: the affine key bytes the caller supplies, or None for [x]G"""
    p, a, b, q, G = S._curve(curve)
    cl, ql = O.clen(curve), O.qlen(curve)
    if not 0 < x < q:
        return 1, 0
    if pub is None:
        pub = bip_pub(curve, x)
    Y = (int.from_bytes(pub[:cl], "big"), int.from_bytes(pub[cl:], "big"))
    if Y[0] >= p or Y[1] >= p or (Y[1] * Y[1] - Y[0] ** 3 - a * Y[0] - b) % p:
        return 1, 0
    d = q - x if Y[1] & 1 else x
    hs = HSIZE[hash_name]
    mask = H(hash_name, S.tagged(hash_name, S.TAG_AUX) + aux.to_bytes(ql, "big"))
    tl = max(ql, hs)
    t = bytes(u ^ v for u, v in zip(d.to_bytes(ql, "big").ljust(tl, b"\0"), mask.ljust(tl, b"\0")))
    k = int.from_bytes(H(hash_name, S.tagged(hash_name, S.TAG_NONCE) + t + pub[:cl] + msg), "big") % q
    return (0, k) if k else (1, 0)


def bip_sign(curve, hash_name, x, aux, msg, pub=None):
    """(status, signature bytes) as ec_bip0340_sign_batch returns them, and the restatement's k"""
    st, k = bip_nonce(curve, hash_name, x, aux, msg, pub)
    return S.sign(curve, S.BIP0340, hash_name, x, k, msg, pub), k


def bip_slot(curve, hash_name, msg, stride, length=None):
    return S.slot(S.BIP0340, hash_name, O.clen(curve), msg, stride, length=length)


def bip_stride(curve, hash_name, max_msg):
    return S.stride_for(S.BIP0340, hash_name, O.clen(curve), max_msg)


def nonce_input_len(curve, hash_name, mlen):
    """octets the nonce hash takes in: H(tag) || H(tag) || t || Y.x || m"""
    hs = HSIZE[hash_name]
    return 2 * hs + max(O.qlen(curve), hs) + O.clen(curve) + mlen


def dbign_edge_hashes(curve):
    """the two hashes under which a curve's x_edge items are recorded: belt-hash and one SHA-2, every one on some curve"""
    return ["BELT", DBIGN_HASHES[1 + DBIGN_CURVES.index(curve) % 4]]


def bip_edge_hashes(curve):
    j = BIP_CURVES.index(curve)
    return [BIP_HASHES[j % 4], BIP_HASHES[(j + 2) % 4]]


DELTA = ("family", "hash", "oid", "t", "msg", "x", "aux")   # fields the file leaves out where the item before has the same


def unpack(items):
    """a curve's items with what the file leaves out put back (tests/golden/make_det_sign_fixture.py:packed)"""
    for j, i in enumerate(items):
        if "msgpat" in i:
            i["msg"] = S.pattern_msg(i.pop("msgpat")).hex()
        for k in DELTA:
            if j and k not in i and k in items[j - 1]:
                i[k] = items[j - 1][k]
        for k, v in (("ret", 0), ("sig", None), ("k", "00" * (len(i["x"]) // 2)), ("rejects", 0), ("y_odd", None)):
            i.setdefault(k, v)
    return items


def load_fixture(path):
    """{"dbign": {curve: [item]}, "bip0340": {curve: [item]}, "dbign_vectors": [item], "bip0340_vectors": [item]}"""
    with open(path) as f:
        fx = json.load(f)
    for kind in ("dbign", "bip0340"):
        for items in fx[kind].values():
            unpack(items)
    return fx
