"""Shared by tests/golden/make_hmac_ht_fixture.py, tests/test_hmac_ht_host.py and tests/test_gpu_hmac_ht.py: the hashes that
ec_hmac_slots_batch, ec_rfc6979_nonce_ht_batch and ec_decdsa_sign_ht_batch serve, the key and message lengths of the known answers, the
items of the deterministic-ECDSA cases (derived from their index, so that the fixture records answers only), the unmodified
reference through ctypes, the host build of libecc_amd/csrc/ecamd_hmac.h, and a Python restatement.

The restatement is hmac.new over hashlib and covers the hashes hashlib has here (hashtable_ref.have_hashlib decides for the ten of
its table; SHA-2 always; SM3 where this OpenSSL has it).  Streebog-256 / -512 and BASH224 / 256 / 384 / 512 have no restatement at all:
for them (and for RIPEMD-160 where OpenSSL has dropped it) the recorded answers of the reference in tests/golden/hmac_ht.json are the
only yardstick."""
import ctypes as C
import hashlib
import hmac
import json
import os
import subprocess

import oracles as O
import hashtable_ref as T

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "hmac_ht.json")
SHIM_SRC = os.path.join(HERE, "hmac_ht_host_shim.cpp")
BUILD = os.path.join(HERE, "_build")

# name: (libecc's hash_alg_type number, digest octets, libecc's block_size, the reference's one-shot, hashlib's name or None)
TABLE = {
    "SHA224": (1, 28, 64, "sha224", "sha224"),
    "SHA256": (2, 32, 64, "sha256", "sha256"),
    "SHA384": (3, 48, 128, "sha384", "sha384"),
    "SHA512": (4, 64, 128, "sha512", "sha512"),
    **T.TABLE,
    "SM3": (11, 32, 64, "sm3", "sm3"),
    "STREEBOG256": (13, 32, 64, "streebog256", None),
    "STREEBOG512": (14, 64, 64, "streebog512", None),
}
HASH_IDS = {name: t[0] for name, t in TABLE.items()}
HASH_SIZES = {name: t[1] for name, t in TABLE.items()}
BLOCKS = {name: t[2] for name, t in TABLE.items()}
NAMES = sorted(TABLE, key=lambda name: HASH_IDS[name])
OLD_NAMES = ["SHA224", "SHA256", "SHA384", "SHA512"]          # what ec_rfc6979_nonce_batch / ec_decdsa_sign_batch serve themselves
NEW_NAMES = [name for name in NAMES if name not in OLD_NAMES]
NOT_SERVED = [0, 12, 16, 21, -1]
N_GPU = 130                                                   # two full waves and a tail of two lanes

DECDSA = 14                                                   # libecc's ec_alg_type number
# SECP192R1: qlen 24 > RIPEMD-160's 20; SECP224K1: qlen 29 and 225 bits; the two Brainpool orders reject candidates; SECP521R1: qlen 66
CURVES = ["SECP192R1", "SECP224K1", "SECP256R1", "BRAINPOOLP256R1", "BRAINPOOLP384R1", "SECP521R1"]
RETRY_CURVE = "BRAINPOOLP256R1"
MAX_RETRIES = 1000


def n_items(curve):
    """recorded items per (curve, hash).  brainpoolP256r1's order is 0.6626 * 2^256, so a candidate is rejected with probability
    0.3374 and at least one of 64 items rejects one with probability 1 - 0.6626^64 = 1 - 4e-12 (derived from the order, not measured)"""
    return 64 if curve == RETRY_CURVE else 8


def have_hashlib(name):
    if name in T.TABLE:
        return T.have_hashlib(name)
    hn = TABLE[name][4]
    if hn is None:
        return False
    try:
        hashlib.new(hn, b"")
    except ValueError:
        return False
    return True


def py_hash(name, data):
    return hashlib.new(TABLE[name][4], data).digest()


def py_hmac(name, key, msg):
    return hmac.new(key, msg, TABLE[name][4]).digest()


# ---- the known answers of HMAC ----
def key_lengths(name):
    """0, 1, around the block; B + 1 and 2 B + 3 take hmac_init's hashed-key branch"""
    b = BLOCKS[name]
    return [0, 1, b - 1, b, b + 1, 2 * b + 3]


def msg_lengths(name):
    """hashtable_ref.kat_lengths without the longest slot: 0, 1, around one and two blocks, and the boundary of the length field"""
    b = BLOCKS[name]
    ls = [0, 1, b - 2, b - 1, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 1]
    if b == 64 and TABLE[name][0] in (1, 2, 11, 15):
        ls += [55, 56]
    if b == 128:
        ls += [111, 112]
    return sorted(set(ls))


def key_bytes(n):
    return bytes((7 * i + 3) & 255 for i in range(n))


def msg_bytes(n):
    return bytes((5 * i + 1) & 255 for i in range(n))


def hmac_pair(name, i):
    """(key length, message length) of item i: the two lists, each walked round and round"""
    kl, ml = key_lengths(name), msg_lengths(name)
    return kl[i % len(kl)], ml[i % len(ml)]


def hmac_pairs(name, n=N_GPU):
    """the distinct pairs among the first n items, in order of appearance"""
    seen, out = set(), []
    for i in range(n):
        p = hmac_pair(name, i)
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


# ---- the deterministic-ECDSA items ----
def derive(curve, name, i):
    """(the key's qlen octets, the message) of item i of a (curve, hash) pair.  Item 0 has the empty message."""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    seed = ("%s/%s/%d" % (curve, name, i)).encode()
    x = 1 + int.from_bytes(hashlib.sha512(b"x" + seed).digest() + hashlib.sha512(b"y" + seed).digest(), "big") % (q - 1)
    mlen = 0 if i == 0 else 1 + (37 * i) % 150
    msg = (hashlib.sha512(b"m" + seed).digest() * 3)[:mlen]
    return x.to_bytes(ql, "big"), msg


def edge_keys(curve):
    """x = 0 (imports and signs), q - 1, q (must not import)"""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    return [x.to_bytes(ql, "big") for x in (0, q - 1, q)]


EDGE_MSG = b"sample"


def bits2int(b, qbits):
    x = int.from_bytes(b, "big")
    return x >> (len(b) * 8 - qbits) if len(b) * 8 > qbits else x


def py_nonce(curve, name, priv, h1):
    """(k, rejected candidates) of __ecdsa_rfc6979_nonce (sig/ecdsa_common.c:48-169) for a hashlib-backed hash; (0, MAX_RETRIES) at the bound"""
    q = O.CURVES[curve]["q"]
    qbits, rlen = q.bit_length(), O.qlen(curve)
    hl = HASH_SIZES[name]
    assert len(priv) == rlen and len(h1) == hl
    bx = priv + (bits2int(h1, qbits) % q).to_bytes(rlen, "big")
    V, K = b"\x01" * hl, b"\x00" * hl
    K = py_hmac(name, K, V + b"\x00" + bx)
    V = py_hmac(name, K, V)
    K = py_hmac(name, K, V + b"\x01" + bx)
    V = py_hmac(name, K, V)
    retries = 0
    while True:
        T_ = b""
        while 8 * len(T_) < qbits:
            V = py_hmac(name, K, V)
            T_ += V
        k = bits2int(T_[:rlen], qbits)
        if k < q:
            return k, retries
        retries += 1
        if retries >= MAX_RETRIES:
            return 0, retries
        K = py_hmac(name, K, V + b"\x00")
        V = py_hmac(name, K, V)


def k_from_sig(curve, priv, h1, sig):
    """the nonce an ECDSA signature was made with: k = s^-1 (e + x r) mod q"""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    r, s = int.from_bytes(sig[:ql], "big"), int.from_bytes(sig[ql:], "big")
    e = bits2int(h1, q.bit_length()) % q
    return pow(s, -1, q) * (e + int.from_bytes(priv, "big") * r) % q


# ---- the unmodified reference -- needs oracle/_ref ----
def ref_hash(name, data):
    L = C.CDLL(O.REF_SO)
    out = C.create_string_buffer(64)
    assert getattr(L, TABLE[name][3])(data, len(data), out) == 0
    return out.raw[:HASH_SIZES[name]]


def ref_hmac(name, key, msg):
    """libecc's hmac() (hash/hmac.c)"""
    L = C.CDLL(O.REF_SO)
    L.hmac.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_char_p, C.c_uint32, C.c_char_p, C.POINTER(C.c_uint8)]
    out, outlen = C.create_string_buffer(64), C.c_uint8(64)
    assert L.hmac(key, len(key), HASH_IDS[name], msg, len(msg), out, C.byref(outlen)) == 0
    assert outlen.value == HASH_SIZES[name]
    return out.raw[:outlen.value]


def ref_sign(curve, name, priv, msg):
    """(ret, signature or None): ec_key_pair_import_from_priv_key_buf + _ec_sign with DECDSA and no `rand` hook, as decdsa_ref.ref_sign;
    ret -2 where the key does not import, -1 where _ec_sign fails"""
    import sigfam_ref as R
    L, params = R.ref_params(curve)
    ql = O.qlen(curve)
    kp = C.create_string_buffer(R.BUF)
    if L.ec_key_pair_import_from_priv_key_buf(kp, params, priv, len(priv), DECDSA) != 0:
        return -2, None
    sig = C.create_string_buffer(2 * ql)
    ret = L._ec_sign(sig, 2 * ql, kp, msg, len(msg), C.cast(None, R.RAND_FN), DECDSA, HASH_IDS[name], None, 0)
    return (0, sig.raw[:2 * ql]) if ret == 0 else (-1, None)


# ---- the fixture ----
N_FULL_MACS, N_FULL_SIGS = 6, 2


def checksum(parts):
    return hashlib.sha256(b"".join(parts)).hexdigest()


def tag(sig):
    return hashlib.sha256(sig).digest()[:4].hex()


def load_fixture():
    """tests/golden/hmac_ht.json, the reference's answers in a compact form (full bytes for the first few, then digests of the rest):
    "hmac":   {hash: {"first": [MAC hex of hmac_pairs(hash)[:N_FULL_MACS] -- every key length once], "all": SHA-256 of all MACs of
              hmac_pairs(hash) in order}}; key = key_bytes(klen), message = msg_bytes(mlen)
    "decdsa": {"CURVE/HASH": {"first": [signature hex of items 0 .. N_FULL_SIGS - 1], "tags": [tag(signature) per item],
              "edges": [the reference's return value per edge_keys(curve) over EDGE_MSG],
              "all": SHA-256 of all item signatures in order, then the signatures of the edges that signed}}; item i is derive(curve, hash, i)"""
    with open(FIXTURE) as f:
        return json.load(f)


def assert_macs(fx, name, mac_of):
    """mac_of: {(key length, message length): MAC} for at least hmac_pairs(name)"""
    rec, pairs = fx["hmac"][name], hmac_pairs(name)
    assert len(rec["first"]) == N_FULL_MACS and {kl for kl, _ in pairs[:N_FULL_MACS]} == set(key_lengths(name))
    for p, h in zip(pairs, rec["first"]):
        assert mac_of[p].hex() == h, (name, p)
    assert checksum([mac_of[p] for p in pairs]) == rec["all"], name


def assert_sigs(fx, curve, name, items, edges):
    """items: [(status, signature)] of derive(curve, name, i) in order; edges: the same for edge_keys(curve) over EDGE_MSG"""
    rec, ql = fx["decdsa"]["%s/%s" % (curve, name)], O.qlen(curve)
    assert len(items) == len(rec["tags"]) == n_items(curve) and len(edges) == 3
    for i, h in enumerate(rec["first"]):
        assert items[i] == (0, bytes.fromhex(h)), (curve, name, i)
    for i, (st, sig) in enumerate(items):
        assert st == 0 and tag(sig) == rec["tags"][i], (curve, name, i)
    for j, ((st, sig), ret) in enumerate(zip(edges, rec["edges"])):
        assert (st == 0) == (ret == 0) and (ret == 0 or sig == bytes(2 * ql)), (curve, name, "edge", j)
    assert checksum([sig for _, sig in items] + [sig for (_, sig), ret in zip(edges, rec["edges"]) if ret == 0]) == rec["all"], (curve, name)


def slot(data, stride, length=None):
    return T.slot(data, stride, length)


def stride_for(maxlen):
    return max(8, (4 + maxlen + 3) & ~3)


# ---- the host build of the unit ----
def build_shim(main=False):
    """tests/hmac_ht_host_shim.cpp as a ctypes library, or (main) as a stand-alone program built with the address and
    undefined-behaviour sanitizers: the path of what was built"""
    os.makedirs(BUILD, exist_ok=True)
    if main:
        exe = os.path.join(BUILD, "hmac_ht_host_asan")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan", "-DHMAC_HT_MAIN", "-o", exe, SHIM_SRC])
        return exe
    so = os.path.join(BUILD, "hmac_ht_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM_SRC])
    return so


_shim = []


def shim():
    if not _shim:
        L = C.CDLL(build_shim())
        u32p = C.POINTER(C.c_uint32)
        L.hh_sizes.argtypes = [C.c_int, C.POINTER(C.c_int)]
        L.hh_hash.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p]
        L.hh_hmac.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, u32p]
        L.hh_slot_hmac.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p]
        L.hh_nonce.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, u32p, u32p]
        _shim.append(L)
    return _shim[0]


def shim_hash(name, data):
    out = C.create_string_buffer(64)
    assert shim().hh_hash(HASH_IDS[name], data, len(data), out) == HASH_SIZES[name]
    return out.raw[:HASH_SIZES[name]]


def shim_hmac(name, key, msg):
    """(MAC, compression / permutation / g_N calls it took)"""
    out, calls = C.create_string_buffer(64), C.c_uint32()
    assert shim().hh_hmac(HASH_IDS[name], key, len(key), msg, len(msg), out, C.byref(calls)) == HASH_SIZES[name]
    return out.raw[:HASH_SIZES[name]], calls.value


def shim_slot_hmac(name, kslot, mslot):
    out = C.create_string_buffer(64)
    assert shim().hh_slot_hmac(HASH_IDS[name], kslot, len(kslot), mslot, len(mslot), out) == HASH_SIZES[name]
    return out.raw[:HASH_SIZES[name]]


def shim_nonce(curve, name, priv, h1):
    """(status, k as qlen octets, rejected candidates, compression / permutation / g_N calls)"""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    out, retries, calls = C.create_string_buffer(ql), C.c_uint32(), C.c_uint32()
    st = shim().hh_nonce(HASH_IDS[name], priv, h1, q.to_bytes(ql, "big"), q.bit_length(), out, C.byref(retries), C.byref(calls))
    return st, out.raw[:ql], retries.value, calls.value
