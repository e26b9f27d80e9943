"""Shared by tests/golden/make_sig_msg_fixture.py, tests/test_sighash2_host.py and tests/test_gpu_sig_msg.py: the hashes of the
message-level ECGDSA / ECRDSA / SM2 entry points (SM3, Streebog-256 / -512 beside SHA-2), message slots, and tests/sigfam_ref.py with
another hash and another SM2 id swapped in.  sigfam_ref.py itself is not edited: `swapped` replaces four of its module attributes
for the length of a `with` block."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import subprocess

import oracles as O
import sigfam_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "sig_msg.json")
SHIM_SRC = os.path.join(HERE, "sighash2_host_shim.cpp")
BUILD = os.path.join(HERE, "_build")

# libecc's hash_alg_type numbers and digest sizes
HASH_IDS = {"SHA224": 1, "SHA256": 2, "SHA384": 3, "SHA512": 4, "SM3": 11, "STREEBOG256": 13, "STREEBOG512": 14}
HASH_SIZES = {"SHA224": 28, "SHA256": 32, "SHA384": 48, "SHA512": 64, "SM3": 32, "STREEBOG256": 32, "STREEBOG512": 64}
REF_ONESHOT = {"SM3": "sm3", "STREEBOG256": "streebog256", "STREEBOG512": "streebog512"}
KAT_LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 4092 - 4]

# (scheme, hash, curve) of the crafted families
COMBOS = [("SM2", "SM3", "SM2P256V1"), ("SM2", "SHA256", "SECP256R1"), ("ECRDSA", "STREEBOG256", "GOST_R3410_2012_256_PARAMSETA"),
          ("ECRDSA", "STREEBOG512", "GOST_R3410_2012_512_PARAMSETA"), ("ECGDSA", "SHA256", "BRAINPOOLP256R1"),
          ("ECGDSA", "STREEBOG512", "SECP256R1")]


def counting(n):
    return bytes(i & 255 for i in range(n))


def ref_hash(hash_name, data):
    """the unmodified reference's one-shot (SM3, Streebog) -- needs oracle/_ref; hashlib for SHA-2, as sigfam_ref does"""
    if hash_name not in REF_ONESHOT:
        return hashlib.new(O.HASHLIB[hash_name], data).digest()
    L = C.CDLL(O.REF_SO)
    out = C.create_string_buffer(64)
    assert getattr(L, REF_ONESHOT[hash_name])(data, len(data), out) == 0
    return out.raw[:HASH_SIZES[hash_name]]


def build_shim(main=False):
    """tests/sighash2_host_shim.cpp as a ctypes library, or (main) as a stand-alone program built with the address and undefined-behaviour
    sanitizers: the path of what was built"""
    os.makedirs(BUILD, exist_ok=True)
    if main:
        exe = os.path.join(BUILD, "sighash2_host_asan")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                               "-DSIGHASH2_MAIN",
                               "-o", exe, SHIM_SRC])
        return exe
    so = os.path.join(BUILD, "sighash2_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM_SRC])
    return so


_shim = []


def shim():
    if not _shim:
        L = C.CDLL(build_shim())
        L.s2_hash.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p]
        L.s2_sm3_streamed.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p]
        L.s2_table_entry.argtypes = [C.c_uint32, C.c_uint32]
        L.s2_table_entry.restype = C.c_uint64
        L.s2_sm2_z.argtypes = [C.c_int, C.c_char_p, C.c_uint32] + [C.c_char_p] * 4 + [C.c_uint32, C.c_char_p, C.c_char_p,
                                                                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _shim.append(L)
    return _shim[0]


def shim_hash(hash_name, data):
    """the project's own host build of the device hash code (SM3, Streebog), hashlib for SHA-2: no reference needed"""
    if hash_name not in REF_ONESHOT:
        return hashlib.new(O.HASHLIB[hash_name], data).digest()
    out = C.create_string_buffer(64)
    assert shim().s2_hash(HASH_IDS[hash_name], data, len(data), out) == HASH_SIZES[hash_name]
    return out.raw[:HASH_SIZES[hash_name]]


def shim_z(hash_name, curve, ident, pub):
    """Z through ecamd_sm2z.h: (Z, octets absorbed on the host, octets of the tail)"""
    c, cl = O.CURVES[curve], O.clen(curve)
    out = C.create_string_buffer(64)
    ab, tl = C.c_uint32(0), C.c_uint32(0)
    n = shim().s2_sm2_z(HASH_IDS[hash_name], ident if ident else None, len(ident), c["a"].to_bytes(cl, "big"), c["b"].to_bytes(cl, "big"),
                        c["gx"].to_bytes(cl, "big"), c["gy"].to_bytes(cl, "big"), cl, pub, out, C.byref(ab), C.byref(tl))
    assert n == HASH_SIZES[hash_name]
    return out.raw[:n], ab.value, tl.value


@contextlib.contextmanager
def swapped(hash_fn, hash_name, ident=S.SM2_ID):
    """sigfam_ref with H = hash_fn(name, data), hashes_for(curve) = [hash_name] and the SM2 id `ident`"""
    saved = (S.H, S.hashes_for, S.SM2_ID, S.sm2_z, dict(O.HASH_IDS))
    orig_z = S.sm2_z
    S.H = hash_fn
    S.hashes_for = lambda curve: [hash_name]
    S.SM2_ID = ident
    S.sm2_z = lambda curve, hn, pub, ident=None: orig_z(curve, hn, pub, S.SM2_ID if ident is None else ident)
    O.HASH_IDS.update(HASH_IDS)
    try:
        yield S
    finally:
        S.H, S.hashes_for, S.SM2_ID, S.sm2_z = saved[:4]
        O.HASH_IDS.clear()
        O.HASH_IDS.update(saved[4])


def pack_slots(msgs, stride, blank=0):
    """message slots: a little-endian u32 length, then `blank` empty octets and the message"""
    out = bytearray(len(msgs) * stride)
    for i, m in enumerate(msgs):
        body = bytes(blank) + m
        assert 4 + len(body) <= stride
        out[i * stride:i * stride + 4] = len(body).to_bytes(4, "little")
        out[i * stride + 4:i * stride + 4 + len(body)] = body
    return bytes(out)


def stride_for(msgs, blank=0):
    return (4 + blank + max(len(m) for m in msgs) + 3) & ~3


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)
