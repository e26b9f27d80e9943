"""CPU tests of batched BIGN / DBIGN: (a) the pure-Python belt-hash and the Python-integer restatement of tests/bign_ref.py against
the recorded reference answers (tests/golden/bign.json) -- this ties the restatement to the reference; (b) belt-hash
(libecc_amd/csrc/ecamd_belt.h) and the per-item steps (libecc_amd/csrc/ecamd_bign.h) through tests/bign_host_shim.cpp (g++, no HIP)
against the restatement and the recording; (c) the whole fixture through a host composition of the steps, with Python-integer
multiplications in the place of the kernels; (d) the new symbols in header, binding and library.

h-bar = 0 and an ACCEPTED u = 0 cannot be reached through the reference, which hashes the message itself (that would invert the
hash): those two rest on the restatement, at the level of the steps, which take the digest from the caller."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libecc_amd
import oracles as O
import bign_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bign.json")
BUILD = os.path.join(ROOT, "tests", "_build")
SHIM = os.path.join(ROOT, "tests", "bign_host_shim.cpp")
SYMBOLS = ["ec_bign_verify_batch", "ec_bign_verify_batch_dev", "ec_bign_sign_batch", "ec_bign_sign_batch_dev"]
CONSTANTS = {"ECAMD_SIG_BIGN": 18, "ECAMD_SIG_DBIGN": 19, "ECAMD_HASH_BELT": 16}
NW = 17
REJECTED = ("s0_bit", "s1_bit", "s0_const", "w_infinity", "key_off_curve", "key_coord_p", "key_small_order")


@pytest.fixture(scope="module")
def fx():
    return B.load_fixture(FIXTURE)


def test_fixture_has_every_family_on_every_curve(fx):
    assert sorted(c for c in fx if c != "belt") == sorted(B.CURVES)
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "sig_hashed.json"))
    assert [n for n, _ in fx["belt"]] == list(range(101)) + [4092]
    for curve in B.CURVES:
        d = fx[curve]
        q, ql, l = O.CURVES[curve]["q"], O.qlen(curve), B.s0_len(curve)
        fams = {}
        for i in d["verify"]:
            fams.setdefault(i["family"], []).append(i["ret"])
        assert {"honest", "s0_bit", "s1_bit", "s1_range", "s0_const", "u_zero", "w_infinity", "doubling", "key_off_curve", "key_coord_p",
                "oid", "msg_len", "other_key"} <= set(fams), (curve, sorted(fams))
        assert ("key_small_order" in fams) == (O.CURVES[curve]["order"] != q)
        assert ("s0_byte32" in fams) == (l > 32)
        # what the issue pins, whatever the restatement says
        assert set(fams["honest"]) == {0} and set(fams["msg_len"]) == {0}
        for f in REJECTED:
            assert set(fams.get(f, [-1])) == {-1}, (curve, f)
        for f in ("s1_range", "oid", "other_key") + (("s0_byte32",) if l > 32 else ()):
            assert set(fams[f]) == {0, -1}, (curve, f)
        assert {i["hash"] for i in d["verify"]} >= set(B.hashes_for(curve))
        assert sorted(len(i["msg"]) // 2 for i in d["verify"] if i["family"] == "msg_len") == sorted(B.MSG_LENS)
        assert {int.from_bytes(bytes.fromhex(i["s1"]), "little") for i in d["verify"] if i["family"] == "s1_range"} >= \
            {0, q - 1, q, (1 << (8 * ql)) - 1}
        assert {len(i["oid"]) // 2 for i in d["verify"] if i["family"] == "oid"} >= {0, 64}
        assert {i["family"] for i in d["sign"]} == {"random", "k_edge", "x_edge", "msg_len", "dbign"}
        assert {int(i["k"], 16) for i in d["sign"] if i["family"] == "k_edge"} == {0, 1, q - 1, q}
        assert {int(i["x"], 16) for i in d["sign"] if i["family"] == "x_edge"} == {0, 1, q - 1, q}
    assert B.s0_len("SECP521R1") == 33 and B.s0_len("SECP224K1") == 14 and O.qlen("SECP224K1") == 29


def test_python_belt_hash_gives_the_recorded_answers(fx):
    for n, dg in fx["belt"]:
        assert B.belt_hash(B.pattern_msg(n)).hex() == dg, n
    if O.have_ref():
        rng = np.random.default_rng(5)
        for n in (0, 1, 31, 32, 33, 63, 64, 65, 259, 1000):
            m = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
            assert B.belt_hash(m) == B.ref_belt_hash(m), n


@pytest.mark.parametrize("curve", B.CURVES)
def test_restatement_gives_the_reference_answers(fx, curve):
    for i in fx[curve]["verify"]:
        args = (curve, i["hash"], bytes.fromhex(i["oid"]), bytes.fromhex(i["pub"]), bytes.fromhex(i["sig"]), bytes.fromhex(i["msg"]))
        assert B.verify(*args) == (0 if i["ret"] == 0 else 1), (curve, i["family"])
    for i in fx[curve]["sign"]:
        st, sig = B.sign(curve, i["hash"], bytes.fromhex(i["oid"]), int(i["x"], 16), int(i["k"], 16), bytes.fromhex(i["msg"]))
        assert st == (0 if i["ret"] == 0 else 1), (curve, i["family"], i["ret"])
        assert sig == (bytes.fromhex(i["out"]) if i["ret"] == 0 else bytes(B.sig_len(curve)))


def test_fixture_is_what_the_reference_says_now():
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_bign_fixture as M
    with open(FIXTURE) as f:
        assert M.dumps(M.build()) == f.read()


# ---- the headers through the shim ----
def words(x):
    return (C.c_uint32 * NW)(*[(x >> (32 * w)) & 0xFFFFFFFF for w in range(NW)])


def from_words(a, off=0):
    return sum(int(a[off + w]) << (32 * w) for w in range(NW))


class Shim:
    def __init__(self, lib, curve):
        q = O.CURVES[curve]["q"]
        self.lib, self.q, self.curve = lib, q, curve
        nw = {8: 8, 12: 12, 17: 17}[min(w for w in (8, 12, 17) if w >= (q.bit_length() + 31) // 32)]
        R = 1 << (32 * nw)
        self.consts = (nw, words(q), words(R * R % q), C.c_uint32((-pow(q, -1, 1 << 32)) % (1 << 32)))
        self.qlen, self.clen = O.qlen(curve), O.clen(curve)

    def verify_uv(self, sig, dg):
        out = (C.c_uint32 * (2 * NW))()
        flag = self.lib.b_verify_uv(*self.consts, sig, self.qlen, dg, len(dg), out)
        return flag, from_words(out), from_words(out, NW)

    def sign_s1(self, x, k, bt, dg):
        out = (C.c_uint32 * NW)()
        st = self.lib.b_sign_s1(*self.consts, words(x), words(k), bt, self.qlen, dg, len(dg), out)
        return st, from_words(out)

    def belt(self, msg):
        stride = B.stride_for(len(msg))
        out = C.create_string_buffer(32)
        self.lib.b_belt_slots(B.slot(msg, stride), stride, 1, out)
        return out.raw

    def t(self, oid, W, dg):
        """fill + belt-hash: the 32 digest bytes"""
        slot = C.create_string_buffer(4 + 64 + 136 + 128 + 4)
        wb = W[0].to_bytes(self.clen, "big") + W[1].to_bytes(self.clen, "big")
        stride = self.lib.b_fill(oid, len(oid), wb, self.clen, self.qlen, dg, len(dg), slot)
        out = C.create_string_buffer(32)
        self.lib.b_belt_slots(slot.raw[:stride], stride, 1, out)
        return out.raw

    # the host composition of the steps, Python integers in the place of the multiplications
    def verify(self, oid, pub, sig, dg):
        p, a, b, q, G = B._curve(self.curve)
        Y = B.import_pub(self.curve, pub)
        flag, u, v = self.verify_uv(sig, dg)
        if Y is None or flag:
            return 1
        W = O.py_add(B.fast_mul(u, G, a, p), B.fast_mul(v, Y, a, p), a, p)
        if W is None:
            return 1
        return 0 if self.lib.b_t_matches(self.t(oid, W, dg), sig, self.qlen) else 1

    def sign(self, oid, x, k, dg):
        p, a, b, q, G = B._curve(self.curve)
        l, tl = self.qlen // 2, min(self.qlen // 2, 32)
        if not 0 < k < q or x >= 1 << (32 * self.consts[0]):
            return 1, bytes(l + self.qlen)
        bt = self.t(oid, B.fast_mul(k, G, a, p), dg)
        st, s1 = self.sign_s1(x, k, bt, dg)
        if st:
            return 1, bytes(l + self.qlen)
        return 0, bt[:tl].ljust(l, b"\0") + s1.to_bytes(self.qlen, "little")


@pytest.fixture(scope="module")
def shimlib():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "bign_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM])
    lib = C.CDLL(so)
    u32p, i, u32 = C.POINTER(C.c_uint32), C.c_int, C.c_uint32
    consts = [i, u32p, u32p, u32]
    lib.b_belt_slots.argtypes = [C.c_char_p, u32, u32, C.c_char_p]
    lib.b_belt_slots.restype = None
    lib.b_verify_uv.argtypes = consts + [C.c_char_p, i, C.c_char_p, i, u32p]
    lib.b_sign_s1.argtypes = consts + [u32p, u32p, C.c_char_p, i, C.c_char_p, i, u32p]
    lib.b_fill.argtypes = [C.c_char_p, u32, C.c_char_p, u32, i, C.c_char_p, u32, C.c_char_p]
    lib.b_fill.restype = u32
    lib.b_t_matches.argtypes = [C.c_char_p, C.c_char_p, i]
    lib.b_slot_ok.argtypes = [u32, u32]
    return lib


def test_belt_hash_header_on_every_length(shimlib, fx):
    # every length 0 .. 259 in 260-byte slots (264 with the length word), one batch
    rng = np.random.default_rng(31)
    msgs = [B.pattern_msg(n) for n in range(101)] + [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in range(101, 260)]
    stride = 264
    out = C.create_string_buffer(32 * len(msgs))
    shimlib.b_belt_slots(b"".join(B.slot(m, stride) for m in msgs), stride, len(msgs), out)
    rec = dict(fx["belt"])
    for n, m in enumerate(msgs):
        got = out.raw[32 * n:32 * n + 32]
        assert got == B.belt_hash(m), n
        if n <= 100:
            assert got.hex() == rec[n], n
        if O.have_ref():
            assert got == B.ref_belt_hash(m), n
    # 4092 bytes in a 4096-byte slot: the bit count crosses the low word boundaries of the counter
    m = B.pattern_msg(4092)
    out = C.create_string_buffer(32)
    shimlib.b_belt_slots(B.slot(m, 4096), 4096, 1, out)
    assert out.raw.hex() == rec[4092] and out.raw == B.belt_hash(m)
    # a length word the slot cannot hold is clamped to the slot
    shimlib.b_belt_slots(B.slot(b"abcd" * 3, 16, length=0xFFFFFFFF), 16, 1, out)
    assert out.raw == B.belt_hash(b"abcd" * 3)


def test_scheme_switches_and_sizes(shimlib):
    assert [a for a in range(0, 24) if shimlib.b_alg_known(a)] == [18, 19]
    assert [shimlib.b_hash_size(t) for t in (0, 1, 2, 3, 4, 5, 15, 16, 17)] == [0, 28, 32, 48, 64, 0, 0, 32, 0]
    for ql in (28, 29, 32, 48, 64, 66):
        assert shimlib.b_s0_len(ql) == ql // 2 and shimlib.b_sig_len(ql) == ql // 2 + ql and shimlib.b_t_len(ql) == min(ql // 2, 32)
    for ln, stride, want in ((0, 4, 1), (1, 4, 0), (252, 256, 1), (253, 256, 0), (0xFFFFFFFF, 256, 0), (4092, 4096, 1), (4093, 4096, 0)):
        assert shimlib.b_slot_ok(ln, stride) == want
    bt = bytes(range(1, 33))
    assert shimlib.b_t_matches(bt, bt[:16], 32) == 1 and shimlib.b_t_matches(bt, bt[:15] + b"\0", 32) == 0
    assert shimlib.b_t_matches(bt, bt + b"\0", 66) == 1 and shimlib.b_t_matches(bt, bt + b"\x01", 66) == 0
    assert shimlib.b_t_matches(bt, bt[:14], 29) == 1


@pytest.mark.parametrize("curve", B.CURVES)
def test_steps_on_the_fixture_and_on_edge_values(shimlib, fx, curve):
    sh = Shim(shimlib, curve)
    p, a, b, q, G = B._curve(curve)
    ql, l = sh.qlen, sh.qlen // 2
    rng = np.random.default_rng(41)
    for i in fx[curve]["verify"]:
        sig, dg = bytes.fromhex(i["sig"]), B.H(i["hash"], bytes.fromhex(i["msg"]))
        assert sh.verify_uv(sig, dg) == B.front_end(curve, sig, dg), (curve, i["family"])
    top = (1 << (8 * ql)) - 1
    for hs in (1, 28, 32, 48, 64, 128):
        dgs = [rng.integers(0, 256, size=hs, dtype=np.uint8).tobytes(), bytes(hs), b"\xff" * hs]
        if q < 1 << (8 * hs):
            dgs += [q.to_bytes(hs, "little"), (q - 1).to_bytes(hs, "little"), (q * (((1 << (8 * hs)) - 1) // q)).to_bytes(hs, "little")]
        for dg in dgs:
            hb = int.from_bytes(dg, "little") % q
            for s1 in (0, 1, q - 1, q, top, (q - hb) % q, B.rand_int(rng, q)):
                for s0 in (bytes(l), b"\xff" * l, rng.integers(0, 256, size=l, dtype=np.uint8).tobytes()):
                    sig = s0 + s1.to_bytes(ql, "little")
                    assert sh.verify_uv(sig, dg) == B.front_end(curve, sig, dg), (curve, hs, s1)
            # signing: s1 for edge keys and nonces, h-bar = 0 among the digests above
            bt = rng.integers(0, 256, size=32, dtype=np.uint8).tobytes()
            s0 = bt[:min(l, 32)].ljust(l, b"\0")
            for x in (0, 1, q - 1, B.rand_int(rng, q)):
                for k in (1, q - 1, B.rand_int(rng, q)):
                    assert sh.sign_s1(x, k, bt, dg) == (0, B.sign_s1(curve, x, k, dg, s0)), (curve, hs, x, k)
            assert sh.sign_s1(q, 1, bt, dg)[0] == 1 and sh.sign_s1(min(top, q + 1), 1, bt, dg)[0] == 1
    # fill + belt-hash against the restatement's t, OIDs of 0, 11 and 64 bytes
    for oid in (b"", B.OID_BELT, bytes(range(64))):
        W = B.fast_mul(1 + B.rand_int(rng, q - 1), G, a, p)
        dg = rng.integers(0, 256, size=int(rng.integers(1, 129)), dtype=np.uint8).tobytes()
        assert sh.t(oid, W, dg)[:min(l, 32)].ljust(l, b"\0") == B.commit_t(curve, oid, W, dg)


@pytest.mark.parametrize("curve", B.CURVES)
def test_whole_fixture_through_the_host_composition(shimlib, fx, curve):
    sh = Shim(shimlib, curve)
    for i in fx[curve]["verify"]:
        dg = B.H(i["hash"], bytes.fromhex(i["msg"]))
        got = sh.verify(bytes.fromhex(i["oid"]), bytes.fromhex(i["pub"]), bytes.fromhex(i["sig"]), dg)
        assert got == (0 if i["ret"] == 0 else 1), (curve, i["family"])
    for i in fx[curve]["sign"]:
        st, sig = sh.sign(bytes.fromhex(i["oid"]), int(i["x"], 16), int(i["k"], 16), B.H(i["hash"], bytes.fromhex(i["msg"])))
        assert st == (0 if i["ret"] == 0 else 1), (curve, i["family"])
        assert sig == (bytes.fromhex(i["out"]) if i["ret"] == 0 else bytes(B.sig_len(curve))), (curve, i["family"])
    # u = 0 accepted: the digest is the caller's
    rng = np.random.default_rng(43)
    item = B.u_zero_accepted(curve, B.OID_BELT, rng, hsize=max(32, sh.qlen))
    pub, sig, dg = item
    assert B.front_end(curve, sig, dg)[1] == 0 and B.verify_digest(curve, B.OID_BELT, pub, sig, dg) == 0
    assert sh.verify(B.OID_BELT, pub, sig, dg) == 0


def test_new_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "libecc_amd.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in libecc_amd.api.EXPORTED_SYMBOLS, sym
    for name, val in CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), header), name
    assert (libecc_amd.api.SIG_BIGN, libecc_amd.api.SIG_DBIGN, libecc_amd.api.HASH_BELT) == (18, 19, 16)
    for m in ("bign_verify", "bign_sign", "bign_verify_dev", "bign_sign_dev"):
        assert hasattr(libecc_amd.api.Curve, m), m
    lib = libecc_amd.api.lib_path()
    if os.path.exists(lib):
        L = C.CDLL(lib)
        for sym in SYMBOLS:
            assert hasattr(L, sym), sym
