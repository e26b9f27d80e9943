"""Shared by tests/golden/make_hash_table_fixture.py, tests/test_hash_table_host.py and tests/test_gpu_hash_table.py: the ten hashes
that ec_digest_slots_batch adds to the device (SHA3-224 / 256 / 384 / 512, SHA-512/224, SHA-512/256, RIPEMD-160, BASH224 / 256 / 384 /
512), their known-answer lengths, the unmodified reference's one-shots, the host build of the per-item units, and message slots."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import oracles as O

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "hash_table.json")
SHIM_SRC = os.path.join(HERE, "hash_table_host_shim.cpp")
BUILD = os.path.join(HERE, "_build")

# name: (libecc's hash_alg_type number, digest octets, block / rate octets, the reference's one-shot, hashlib's name or None)
TABLE = {
    "SHA3_224": (5, 28, 144, "sha3_224", "sha3_224"),
    "SHA3_256": (6, 32, 136, "sha3_256", "sha3_256"),
    "SHA3_384": (7, 48, 104, "sha3_384", "sha3_384"),
    "SHA3_512": (8, 64, 72, "sha3_512", "sha3_512"),
    "SHA512_224": (9, 28, 128, "sha512_224", "sha512_224"),
    "SHA512_256": (10, 32, 128, "sha512_256", "sha512_256"),
    "RIPEMD160": (15, 20, 64, "ripemd160", "ripemd160"),
    "BASH224": (17, 28, 136, "bash224", None),
    "BASH256": (18, 32, 128, "bash256", None),
    "BASH384": (19, 48, 96, "bash384", None),
    "BASH512": (20, 64, 64, "bash512", None),
}
HASH_IDS = {name: t[0] for name, t in TABLE.items()}
HASH_SIZES = {name: t[1] for name, t in TABLE.items()}
BLOCKS = {name: t[2] for name, t in TABLE.items()}
MAX_LEN = 4092                                       # the longest message a slot holds (stride 4096)
# the numbers ec_hash_slots_batch serves already, and everything ec_digest_slots_batch serves
OLD_IDS = {1: 28, 2: 32, 3: 48, 4: 64, 11: 32, 13: 32, 14: 64}
ALL_SIZES = {**OLD_IDS, **{t[0]: t[1] for t in TABLE.values()}}

# BIGN's OIDs of bash384 and bash512 (1.2.112.0.2.0.34.101.77.12 / .13)
OID_BASH = {"BASH384": bytes.fromhex("06092A7000020022654D0C"), "BASH512": bytes.fromhex("06092A7000020022654D0D")}
ECDSA, BIGN, DBIGN = 1, 18, 19                       # libecc's ec_alg_type numbers
# (scheme, curve, hash) of the recorded protocol items
COMBOS = [("BIGN", "BIGN384V1", "BASH384"), ("BIGN", "BIGN512V1", "BASH512"), ("DBIGN", "BIGN384V1", "BASH384"),
          ("ECDSA", "SECP256R1", "SHA3_256"), ("ECDSA", "SECP384R1", "SHA3_384")]


def counting(n):
    return bytes(i & 255 for i in range(n))


def kat_lengths(name):
    """0, 1, the lengths around one and two blocks, the longest a slot holds; for the hashes with a length field its boundary too"""
    b = BLOCKS[name]
    ls = [0, 1, b - 2, b - 1, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 1, MAX_LEN]
    if name == "RIPEMD160":
        ls += [55, 56]
    if name.startswith("SHA512_"):
        ls += [111, 112]
    return sorted(set(ls))


def have_hashlib(name):
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


def ref_hash(name, data):
    """the unmodified reference's one-shot -- needs oracle/_ref"""
    L = C.CDLL(O.REF_SO)
    out = C.create_string_buffer(64)
    assert getattr(L, TABLE[name][3])(data, len(data), out) == 0
    return out.raw[:HASH_SIZES[name]]


def build_shim(main=False):
    """tests/hash_table_host_shim.cpp as a ctypes library, or (main) as a stand-alone program built with the address and
    undefined-behaviour sanitizers: the path of what was built"""
    os.makedirs(BUILD, exist_ok=True)
    if main:
        exe = os.path.join(BUILD, "hash_table_host_asan")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan", "-DHASH_TABLE_MAIN", "-o", exe, SHIM_SRC])
        return exe
    so = os.path.join(BUILD, "hash_table_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM_SRC])
    return so


_shim = []


def shim():
    if not _shim:
        L = C.CDLL(build_shim())
        L.ht_sizes.argtypes = [C.c_int, C.POINTER(C.c_int)]
        L.ht_hash.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p]
        L.ht_slot.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p]
        L.ht_bash_rc.argtypes = [C.c_uint32]
        L.ht_bash_rc.restype = C.c_uint64
        _shim.append(L)
    return _shim[0]


def shim_hash(name, data):
    """the project's own host build of the device hash code"""
    out = C.create_string_buffer(64)
    assert shim().ht_hash(HASH_IDS[name], data, len(data), out) == HASH_SIZES[name]
    return out.raw[:HASH_SIZES[name]]


def slot(msg, stride, length=None):
    """a message slot: a little-endian u32 length (`length`: a field that does not tell the truth), then the message"""
    assert 4 + len(msg) <= stride and stride % 4 == 0
    return (len(msg) if length is None else length).to_bytes(4, "little") + msg + bytes(stride - 4 - len(msg))


def pack_slots(msgs, stride):
    return b"".join(slot(m, stride) for m in msgs)


def stride_for(msgs):
    return (4 + max(len(m) for m in msgs) + 3) & ~3


def load_fixture():
    """tests/golden/hash_table.json: {"kats": {hash: [[length, digest hex]]}, "items": {"SCHEME/CURVE/HASH": [item]}}"""
    with open(FIXTURE) as f:
        return json.load(f)


def kat_table(fx):
    """{hash: {length: digest bytes}}"""
    return {name: {n: bytes.fromhex(h) for n, h in rows} for name, rows in fx["kats"].items()}
