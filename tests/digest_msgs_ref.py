"""Shared by tests/golden/make_digest_msgs_fixture.py, tests/test_digest_msgs_host.py and tests/test_gpu_digest_msgs.py: the cases of
ec_digest_msgs_batch (total lengths around every block and length-field boundary, each split over call prefix, item prefix and message),
the protocol items of ec_ecdsa_verify_msgs_batch / ec_decdsa_sign_msgs_batch, the host build of libecc_amd/csrc/ecamd_digest_msgs.h, and
the compact fixture tests/golden/digest_msgs.json.  Messages are generated from a seed (SHAKE256 of the case's name); the fixture
records the unmodified reference's answers only."""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess

import oracles as O
import hmac_ht_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "digest_msgs.json")
SHIM_SRC = os.path.join(HERE, "digest_msgs_host_shim.cpp")
BUILD = os.path.join(HERE, "_build")

NAMES = M.NAMES                       # the 18 served hashes, by libecc's number
HASH_IDS, HASH_SIZES, BLOCKS = M.HASH_IDS, M.HASH_SIZES, M.BLOCKS
MAX_PREFIX = 256
MAX_HASHED = 1 << 28
LONG = 70001
N_GPU = 130                           # two full waves and a tail of two lanes
VARIANTS = 4                          # splits per total length


def length_field(name):
    """octets the padding needs behind the message beside its first octet: the bit count of the Merkle-Damgard hashes (8, or 16 on
    1024-bit blocks); SHA-3, BASH and Streebog pad with one octet that may be the block's last, which the lengths below express as 1"""
    hid = HASH_IDS[name]
    if hid in (1, 2, 11, 15):
        return 8
    if hid in (3, 4, 9, 10):
        return 16
    return 1


def totals(name):
    b, l = BLOCKS[name], length_field(name)
    return sorted({0, 1, 3, 4, 5, b - l - 2, b - l - 1, b - l, b - 1, b, b + 1, 2 * b - l - 1, 2 * b - l, 2 * b, 4092, 4093, 4097, LONG})


def stream(tag, n):
    """n octets from a seed"""
    return hashlib.shake_256(tag.encode()).digest(n) if n else b""


def cases(name):
    """[(total, call prefix length, item prefix length)]: variant 0 of every total is the message alone; the others split it at seeded
    places.  With a total of 0 all three segments are empty."""
    rng = random.Random("digest_msgs/" + name)
    out = []
    for t in totals(name):
        out.append((t, 0, 0))
        for v in range(1, VARIANTS):
            cpl = rng.randint(0, min(t, MAX_PREFIX))
            ipl = rng.randint(0, min(t - cpl, MAX_PREFIX))
            if v == 1 and 0 < t <= 2 * MAX_PREFIX:          # the whole input in the prefixes: an empty message behind them
                cpl = t // 2
                ipl = t - cpl
            out.append((t, cpl, ipl))
    return out


def case_stream(name, idx):
    """the octets case idx hashes.  The first MAX_PREFIX octets are the same for every case of a hash, so that cases can share one call
    prefix in a batch; what follows is the case's own."""
    t = cases(name)[idx][0]
    return stream("digest_msgs/%s/common" % name, min(t, MAX_PREFIX)) + stream("digest_msgs/%s/%d" % (name, idx), max(0, t - MAX_PREFIX))


def case_input(name, idx):
    """(call prefix, item prefix, message) of case idx"""
    t, cpl, ipl = cases(name)[idx]
    x = case_stream(name, idx)
    return x[:cpl], x[cpl:cpl + ipl], x[cpl + ipl:]


# (call prefix length, item prefix length) of the batches the device tests run: a digest depends on the octets only, not on where they
# are cut, so one batch cuts every case that is long enough at the same two places
GPU_SPLITS = [(0, 0), (5, 3), (2, 65), (255, 6), (256, 256)]


def batch(name, cpl, ipl, n=N_GPU):
    """(case indices, call prefix, item prefixes, messages) of n items: the cases of at least cpl + ipl octets, walked round and round"""
    idxs = [i for i, c in enumerate(cases(name)) if c[0] >= cpl + ipl]
    idxs = [idxs[k % len(idxs)] for k in range(n)]
    xs = {i: case_stream(name, i) for i in set(idxs)}
    cp = stream("digest_msgs/%s/common" % name, cpl)
    assert all(xs[i][:cpl] == cp for i in idxs)
    return idxs, cp, [xs[i][cpl:cpl + ipl] for i in idxs], [xs[i][cpl + ipl:] for i in idxs]


def coverage(name):
    """what the splits reach: the residues mod 4 of each segment's length"""
    cs = cases(name)
    return ({c[1] & 3 for c in cs}, {c[2] & 3 for c in cs}, {(c[0] - c[1] - c[2]) & 3 for c in cs})


# ---- the protocol items ----
PROTO = [("SECP256R1", "SHA3_256"), ("BRAINPOOLP384R1", "SHA512_256"), ("SECP521R1", "RIPEMD160")]
PROTO_LENS = [0, 1, 150, 4093, 9000, LONG]


def proto_item(curve, name, i):
    """(private key octets, affine public key, message) of item i"""
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    seed = "digest_msgs/proto/%s/%s/%d" % (curve, name, i)
    x = 1 + int.from_bytes(stream(seed + "/x", 80), "big") % (q - 1)
    return x.to_bytes(ql, "big"), O.py_smul_bytes(curve, x), stream(seed + "/m", PROTO_LENS[i])


def flip_sig(sig):
    return sig[:-1] + bytes([sig[-1] ^ 1])


def flip_msg(msg):
    """a flipped bit in the last octet; the empty message grows by one octet instead (it has no bit to flip)"""
    return msg[:-1] + bytes([msg[-1] ^ 0x80]) if msg else b"\x80"


ECDSA = 1   # libecc's ec_alg_type number


def ref_verify(curve, name, pub, sig, msg):
    """the unmodified reference -- needs oracle/_ref: ec_pub_key_import_from_aff_buf + ec_verify with ECDSA, 0 / -1"""
    import sigfam_ref as R
    L, params = R.ref_params(curve)
    key = C.create_string_buffer(R.BUF)
    if L.ec_pub_key_import_from_aff_buf(key, params, pub, len(pub), ECDSA) != 0:
        return -1
    return -1 if L.ec_verify(sig, len(sig), key, msg, len(msg), ECDSA, HASH_IDS[name], None, 0) != 0 else 0


# ---- the fixture ----
TAG = 8


def tag(d):
    return d[:TAG].hex()


def checksum(parts):
    return hashlib.sha256(b"".join(parts)).hexdigest()


def load_fixture():
    """tests/golden/digest_msgs.json:
    "digests": {hash: {"full": [digest hex of variant 0 of every total, in order], "tags": [the first 8 octets of every case's digest],
               "all": SHA-256 over all digests of cases(hash) in order}}
    "proto":   {"CURVE/HASH": {"sigs": [DECDSA signature hex per message], "verdicts": [[honest, flipped signature bit, flipped message
               bit] per message]}}
    "sha256":  SHA-256 over every "all" and every signature in order"""
    with open(FIXTURE) as f:
        return json.load(f)


def assert_digests(fx, name, digs):
    """digs: the digests of cases(name) in order"""
    rec, cs = fx["digests"][name], cases(name)
    assert len(digs) == len(cs) == len(rec["tags"]) == VARIANTS * len(totals(name))
    full =[digs[VARIANTS * k] for k in range(len(totals(name)))]
    assert [d.hex() for d in full] == rec["full"], name
    for i, d in enumerate(digs):
        assert len(d) == HASH_SIZES[name] and tag(d) == rec["tags"][i], (name, i, cs[i])
    assert checksum(digs) == rec["all"], name


# ---- the host build of the unit ----
def build_shim(main=False):
    """tests/digest_msgs_host_shim.cpp as a ctypes library, or (main) as a stand-alone program built with the address and
    undefined-behaviour sanitizers: the path of what was built"""
    os.makedirs(BUILD, exist_ok=True)
    if main:
        exe = os.path.join(BUILD, "digest_msgs_host_asan")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan", "-DDIGEST_MSGS_MAIN", "-o", exe, SHIM_SRC])
        return exe
    so = os.path.join(BUILD, "digest_msgs_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM_SRC])
    return so


_shim = []


def shim():
    if not _shim:
        L = C.CDLL(build_shim())
        u64 = C.c_uint64
        L.dm_item_ok.argtypes = [u64, u64, u64, C.c_uint32, C.c_uint32]
        L.dm_digest.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, u64, u64, u64, C.c_char_p]
        _shim.append(L)
    return _shim[0]


def shim_digest(name, cp, ip, arr, off0, off1, total=None):
    """(status, digest) of the unit for the item arr[off0 .. off1) of an array of `total` octets (default: all of arr)"""
    out = C.create_string_buffer(64)
    st = shim().dm_digest(HASH_IDS[name], cp, len(cp), ip, len(ip), arr, off0, off1, len(arr) if total is None else total, out)
    assert st in (0, 1), st
    return st, out.raw[:HASH_SIZES[name]]
