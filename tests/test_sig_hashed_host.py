"""CPU tests of batched ECSDSA / ECOSDSA / ECKCDSA: (a) the recorded reference answers (tests/golden/sig_hashed.json) against the
Python-integer restatement of tests/sighash_ref.py, item for item -- this ties the restatement to the reference; (b) the
field-level steps of libecc_amd/csrc/ecamd_sighash.h through tests/sig_hashed_host_shim.cpp (g++, no HIP) against the
restatement, on the fixture inputs and on random and edge values of every q length -- among them inputs the reference cannot be
driven to through a real hash (r = 0 mod q for every digest size, ECKCDSA's e = 0, s = 0 in signing): THOSE REST ON THE
RESTATEMENT; (c) the new symbols in header, binding and library."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libecc_amd
import oracles as O
import sighash_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sig_hashed.json")
BUILD = os.path.join(ROOT, "tests", "_build")
SHIM = os.path.join(ROOT, "tests", "sig_hashed_host_shim.cpp")
SYMBOLS = ["ec_sig_hashed_verify_batch", "ec_sig_hashed_verify_batch_dev", "ec_sig_hashed_sign_batch", "ec_sig_hashed_sign_batch_dev"]
CONSTANTS = {"ECAMD_SIG_ECKCDSA": 2, "ECAMD_SIG_ECSDSA": 3, "ECAMD_SIG_ECOSDSA": 4}
NW = 17
REJECTED = ("tampered", "s_range", "w_infinity", "key_not_importable", "key_small_order", "key_torsion", "foreign_scheme")


def load_fixture():
    return S.load_fixture(FIXTURE)


def test_fixture_has_every_family_on_every_curve_and_scheme():
    fx = load_fixture()
    assert sorted(fx) == sorted(S.CURVES)
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "sig_family.json"))
    for curve, per in fx.items():
        assert sorted(per) == sorted(S.SCHEMES)
        q, ql = O.CURVES[curve]["q"], O.qlen(curve)
        for name, d in per.items():
            alg = S.SCHEMES[name]
            fams = {i["family"] for i in d["verify"]}
            assert {"honest", "tampered", "s_range", "r_zero_mod_q", "w_infinity", "equal_operands", "key_not_importable", "pad_edges",
                    "longest", "foreign_scheme"} <= fams, (curve, name, fams)
            assert ("e_zero" in fams) == (alg == S.ECKCDSA)
            assert ({"key_small_order", "key_torsion"} <= fams) == (O.CURVES[curve]["order"] != q)
            assert {i["hash"] for i in d["verify"]} >= set(S.hashes_for(curve))
            assert {i["family"] for i in d["sign"]} == {"honest", "x_edge", "k_edge", "pad_edges"}
            for i in d["verify"]:
                # what the issue pins, whatever the restatement says
                if i["family"] in ("honest", "pad_edges", "longest"):
                    assert i["ret"] == 0, (curve, name, i["family"])
                if i["family"] in REJECTED or (i["family"] == "r_zero_mod_q" and alg != S.ECKCDSA):
                    assert i["ret"] == -1, (curve, name, i["family"])
            if alg != S.ECKCDSA:
                lens = sorted(len(i["msg"]) // 2 for i in d["verify"] if i["family"] == "pad_edges")
                assert lens == sorted(S.PAD_EDGES)
                assert [len(i["msg"]) // 2 for i in d["verify"] if i["family"] == "longest"] == [4096 - 4 - S.blank_len(alg, O.clen(curve))]
            # s = 0, q, q - 1 and k = 0, q, q - 1, x = 0, q - 1, >= q
            assert {int(i["s"], 16) for i in d["verify"] if i["family"] == "s_range"} >= {0, q, q - 1}
            assert {int(i["k"], 16) for i in d["sign"] if i["family"] == "k_edge"} >= {0, q, q - 1}
            assert {int(i["x"], 16) for i in d["sign"] if i["family"] == "x_edge"} >= {0, q - 1, q}
    # the truncation cases of ECKCDSA: shift 3, 32, 16 and hsize < qlen
    shifts = {(c, i["hash"]): max(0, S.HSIZE[i["hash"]] - O.qlen(c)) for c in fx for i in fx[c]["ECKCDSA"]["verify"]}
    assert shifts[("SECP224K1", "SHA256")] == 3 and shifts[("SECP256R1", "SHA512")] == 32 and shifts[("SECP384R1", "SHA512")] == 16
    assert shifts[("SECP521R1", "SHA224")] == 0 and shifts[("SECP384R1", "SHA256")] == 0 and shifts[("SECP256K1", "SHA256")] == 0


@pytest.mark.parametrize("curve", S.CURVES)
def test_restatement_gives_the_reference_answers(curve):
    fx = load_fixture()[curve]
    ql = O.qlen(curve)
    for name, alg in S.SCHEMES.items():
        for i in fx[name]["verify"]:
            pub, sig, msg = bytes.fromhex(i["pub"]), bytes.fromhex(i["sig"]), bytes.fromhex(i["msg"])
            assert S.verify(curve, alg, i["hash"], pub, sig, msg) == (0 if i["ret"] == 0 else 1), (curve, name, i["family"])
        for i in fx[name]["sign"]:
            st, sig = S.sign(curve, alg, i["hash"], int(i["x"], 16), int(i["k"], 16), bytes.fromhex(i["msg"]))
            assert st == (0 if i["ret"] == 0 else 1), (curve, name, i["family"], i["ret"])
            assert sig == (bytes.fromhex(i["out"]) if i["ret"] == 0 else bytes(S.r_len(alg, i["hash"], ql) + ql))


def test_fixture_is_what_the_reference_says_now():
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_sig_hashed_fixture as M
    with open(FIXTURE) as f:
        assert M.dumps(M.build()) == f.read()


# ---- the header through the shim ----
def words(x):
    return (C.c_uint32 * NW)(*[(x >> (32 * w)) & 0xFFFFFFFF for w in range(NW)])


def from_words(a, off=0):
    return sum(int(a[off + w]) << (32 * w) for w in range(NW))


class Shim:
    def __init__(self, lib, q):
        self.lib, self.q = lib, q
        nw = {8: 8, 12: 12, 17: 17}[(q.bit_length() + 31) // 32]
        R = 1 << (32 * nw)
        self.consts = (nw, words(q), words(R * R % q), C.c_uint32((-pow(q, -1, 1 << 32)) % (1 << 32)))
        self.qlen = (q.bit_length() + 7) // 8

    def verify_uv(self, alg, sig, hsize, h):
        out = (C.c_uint32 * (2 * NW))()
        flag = self.lib.h_verify_uv(*self.consts, alg, sig, hsize, self.qlen, h, out)
        return flag, from_words(out), from_words(out, NW)

    def sign_s(self, alg, x, k, dg, h):
        out = (C.c_uint32 * NW)()
        st = self.lib.h_sign_s(*self.consts, alg, words(x), words(k), dg, len(dg), self.qlen, h, out)
        return st, from_words(out)


@pytest.fixture(scope="module")
def shimlib():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "sig_hashed_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM])
    lib = C.CDLL(so)
    u32p, i = C.POINTER(C.c_uint32), C.c_int
    consts = [i, u32p, u32p, C.c_uint32]
    lib.h_verify_uv.argtypes = consts + [i, C.c_char_p, i, i, C.c_char_p, u32p]
    lib.h_sign_s.argtypes = consts + [i, u32p, u32p, C.c_char_p, i, i, C.c_char_p, u32p]
    lib.h_slot_ok.argtypes = [i, C.c_uint32, C.c_uint32, i]
    lib.h_digest_matches.argtypes = [C.c_char_p, i, C.c_char_p, i]
    return lib


def py_uv(alg, q, ql, sig, hsize, h):
    """the restatement of verify_uv on raw bytes (h given, not derived from a key)"""
    rl = min(hsize, ql) if alg == S.ECKCDSA else hsize
    r, s = sig[:rl], int.from_bytes(sig[rl:], "big")
    if not 0 < s < q:
        return 1, 0, 0
    if alg == S.ECKCDSA:
        return 0, S.kcdsa_e(r, h, q), s
    e = -int.from_bytes(r, "big") % q
    return (1, 0, 0) if e == 0 else (0, s, e)


def py_s(alg, q, ql, x, k, dg, h):
    rl = min(len(dg), ql) if alg == S.ECKCDSA else len(dg)
    if not S.key_ok(alg, q, x):
        return 2, 0
    if alg == S.ECKCDSA:
        s = x * (k - S.kcdsa_e(dg[len(dg) - rl:], h, q)) % q
        return (0 if s else 1), s
    e = int.from_bytes(dg, "big") % q
    s = (k + e * x) % q
    return (0 if e and s else 1), s


def test_scheme_switches_and_sizes(shimlib):
    assert [shimlib.h_alg_known(a) for a in range(0, 10)] == [0, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert [shimlib.h_hash_size(t) for t in range(0, 7)] == [0, 28, 32, 48, 64, 0, 0]
    for ql in (28, 29, 32, 48, 66):
        for hs in (28, 32, 48, 64):
            assert shimlib.h_r_len(S.ECKCDSA, hs, ql) == min(hs, ql)
            assert shimlib.h_r_len(S.ECSDSA, hs, ql) == hs and shimlib.h_r_len(S.ECOSDSA, hs, ql) == hs
    assert shimlib.h_blank_len(S.ECSDSA, 32) == 64 and shimlib.h_blank_len(S.ECOSDSA, 32) == 32 and shimlib.h_blank_len(S.ECSDSA, 66) == 132
    # a slot: the blank is counted in the length, and 4 + length <= stride
    for alg, bl in ((S.ECSDSA, 64), (S.ECOSDSA, 32)):
        for ln, stride, want in ((bl, 4 + bl, 1), (bl - 1, 256, 0), (0, 256, 0), (252, 256, 1), (253, 256, 0), (0xFFFFFFFF, 256, 0),
                                 (4092, 4096, 1), (4093, 4096, 0)):
            assert shimlib.h_slot_ok(alg, ln, stride, 32) == want, (alg, ln, stride)
    dg = bytes(range(64))
    assert shimlib.h_digest_matches(dg, 64, dg, 64) == 1 and shimlib.h_digest_matches(dg, 64, dg[32:], 32) == 1
    assert shimlib.h_digest_matches(dg, 64, dg[:32], 32) == 0 and shimlib.h_digest_matches(dg, 64, dg[31:63], 32) == 0


@pytest.mark.parametrize("curve", S.CURVES)
def test_front_end_on_random_and_edge_values(shimlib, curve):
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    sh = Shim(shimlib, q)
    rng = np.random.default_rng(77)
    top = (1 << (8 * ql)) - 1
    for hs in (28, 32, 48, 64):
        rs = [rng.integers(0, 256, size=hs, dtype=np.uint8).tobytes() for _ in range(6)] + [bytes(hs), b"\xff" * hs]
        rs += [(q * m).to_bytes(hs, "big") for m in (1, 2, ((1 << (8 * hs)) - 1) // q) if q * m < (1 << (8 * hs))]
        rs += [(q * m + d).to_bytes(hs, "big") for m in (0, 1) for d in (1, q - 1) if q * m + d < (1 << (8 * hs))]
        for r in rs:
            h = rng.integers(0, 256, size=hs, dtype=np.uint8).tobytes()
            for s in (0, 1, q - 1, q, min(top, q + 1), top, S.rand_int(rng, q)):
                for alg in S.SCHEMES.values():
                    rl = min(hs, ql) if alg == S.ECKCDSA else hs
                    sig = r[hs - rl:] + s.to_bytes(ql, "big")
                    assert sh.verify_uv(alg, sig, hs, h) == py_uv(alg, q, ql, sig, hs, h), (curve, alg, hs, s)
            # ECKCDSA's e = 0 (r = h') is allowed, and e = q exactly where it fits
            rl = min(hs, ql)
            assert sh.verify_uv(S.ECKCDSA, h[hs - rl:] + (5).to_bytes(ql, "big"), hs, h) == (0, 0, 5)
            if q < (1 << (8 * rl)):
                rq = bytes(a ^ b for a, b in zip(q.to_bytes(rl, "big"), h[hs - rl:]))
                assert sh.verify_uv(S.ECKCDSA, rq + (5).to_bytes(ql, "big"), hs, h) == (0, 0, 5)


@pytest.mark.parametrize("curve", S.CURVES)
def test_signing_back_end_on_random_and_edge_values(shimlib, curve):
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    sh = Shim(shimlib, q)
    rng = np.random.default_rng(78)
    top = (1 << (8 * ql)) - 1
    for hs in (28, 32, 48, 64):
        for _ in range(4):
            dg = rng.integers(0, 256, size=hs, dtype=np.uint8).tobytes()
            h = rng.integers(0, 256, size=hs, dtype=np.uint8).tobytes()
            k = 1 + S.rand_int(rng, q - 1)
            for x in (0, 1, q - 1, q, min(top, q + 1), top, S.rand_int(rng, q)):
                for alg in S.SCHEMES.values():
                    assert sh.sign_s(alg, x, k, dg, h) == py_s(alg, q, ql, x, k, dg, h), (curve, alg, hs, x)
        # the failures no real hash reaches: e = 0 (ECSDSA), s = 0 (k = -e x; ECKCDSA k = e)
        x = 1 + S.rand_int(rng, q - 1)
        zero = (q * (((1 << (8 * hs)) - 1) // q)).to_bytes(hs, "big")
        for alg in (S.ECSDSA, S.ECOSDSA):
            assert sh.sign_s(alg, x, 7, zero, None)[0] == 1 and sh.sign_s(alg, x, 7, bytes(hs), None)[0] == 1
            dg = rng.integers(0, 256, size=hs, dtype=np.uint8).tobytes()
            e = int.from_bytes(dg, "big") % q
            assert sh.sign_s(alg, x, -e * x % q, dg, None) == (1, 0)
        dg = rng.integers(0, 256, size=hs, dtype=np.uint8).tobytes()
        h = rng.integers(0, 256, size=hs, dtype=np.uint8).tobytes()
        e = S.kcdsa_e(dg[hs - min(hs, ql):], h, q)
        assert sh.sign_s(S.ECKCDSA, x, e, dg, h) == (1, 0)
        assert sh.sign_s(S.ECKCDSA, x, (e + 1) % q, dg, h) == (0, x)


@pytest.mark.parametrize("curve", S.CURVES)
def test_header_on_the_fixture_inputs(shimlib, curve):
    fx = load_fixture()[curve]
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    sh = Shim(shimlib, q)
    for name, alg in S.SCHEMES.items():
        for i in fx[name]["verify"]:
            pub, sig, msg = bytes.fromhex(i["pub"]), bytes.fromhex(i["sig"]), bytes.fromhex(i["msg"])
            h = S.kcdsa_h(curve, i["hash"], pub, msg) if alg == S.ECKCDSA else None
            assert sh.verify_uv(alg, sig, S.HSIZE[i["hash"]], h) == S.front_end(curve, alg, i["hash"], pub, sig, msg), (name, i["family"])


def test_new_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "libecc_amd.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in libecc_amd.api.EXPORTED_SYMBOLS, sym
    for name, val in CONSTANTS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), header), name
    assert (libecc_amd.api.SIG_ECKCDSA, libecc_amd.api.SIG_ECSDSA, libecc_amd.api.SIG_ECOSDSA) == (2, 3, 4)
    for m in ("sig_hashed_verify", "sig_hashed_sign", "sig_hashed_verify_dev", "sig_hashed_sign_dev"):
        assert hasattr(libecc_amd.api.Curve, m), m
    lib = libecc_amd.api.lib_path()
    if os.path.exists(lib):
        L = C.CDLL(lib)
        for sym in SYMBOLS:
            assert hasattr(L, sym), sym
