"""CPU tests of batched ECGDSA / ECRDSA / SM2: (a) the recorded reference answers (tests/golden/sig_family.json) against the
Python-integer restatement of tests/sigfam_ref.py, item for item -- this ties the restatement to the reference; (b) the field-level
steps of libecc_amd/csrc/ecamd_sigfam.h through tests/sig_family_host_shim.cpp (g++, no HIP) against the restatement, on the
fixture inputs AND on inputs the reference cannot be driven to through a real hash: e = 0 mod q (ECRDSA's 0 -> 1, SM2 with
target = r, ECGDSA u = 0), every digest length 1 .. 128, SM2's r + k = q.  THOSE LAST CASES REST ON THE RESTATEMENT, NOT ON THE
REFERENCE; (c) the new symbols in header, binding and library."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libecc_amd
import oracles as O
import sigfam_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sig_family.json")
BUILD = os.path.join(ROOT, "tests", "_build")
SHIM = os.path.join(ROOT, "tests", "sig_family_host_shim.cpp")
SYMBOLS = ["ec_sig_verify_batch", "ec_sig_verify_batch_dev", "ec_sig_sign_batch", "ec_sig_sign_batch_dev"]
NW = 17   # words per array at the shim's boundary
VERIFY_FAMILIES = ["honest", "tampered", "range", "w_infinity", "opposite_operands", "equal_operands", "key_not_importable"]


def load_fixture():
    return S.load_fixture(FIXTURE)


def test_fixture_has_every_family_on_every_curve_and_scheme():
    fx = load_fixture()
    assert sorted(fx) == sorted(S.CURVES)
    for curve, per in fx.items():
        assert sorted(per) == sorted(S.SCHEMES)
        q, p = O.CURVES[curve]["q"], O.CURVES[curve]["p"]
        for name, d in per.items():
            fams = {i["family"] for i in d["verify"]}
            assert set(VERIFY_FAMILIES) <= fams, (curve, name, fams)
            assert ("t_zero" in fams) == (name == "SM2")
            assert ({"key_small_order", "key_torsion"} <= fams) == (O.CURVES[curve]["order"] != q)
            # r + q is there wherever it fits the signature's bytes for some honest r
            if q + (q >> 2) < (1 << (8 * O.qlen(curve))):
                assert "r_plus_q" in fams, (curve, name)
            assert {i["hash"] for i in d["verify"]} >= set(S.hashes_for(curve))
            assert {i["family"] for i in d["sign"]} == {"honest", "x_edge", "k_edge"}
            for i in d["verify"]:
                # what the issue pins, whatever the restatement says
                if i["family"] == "honest":
                    assert i["ret"] == 0, (curve, name, i)
                if i["family"] in ("tampered", "range", "r_plus_q", "w_infinity", "opposite_operands", "t_zero", "key_not_importable",
                                   "key_small_order", "key_torsion"):
                    assert i["ret"] == -1, (curve, name, i)
            # an accepted doubling ([u]G = [v]Y) exists for ECRDSA, where the key can be chosen after e
            if name == "ECRDSA":
                assert any(i["ret"] == 0 for i in d["verify"] if i["family"] == "equal_operands"), curve
            assert sum(i["ret"] == 0 for i in d["sign"]) >= 6
    # digests shorter than, as long as and longer than q
    assert {len(i["digest"]) // 2 for i in fx["SECP521R1"]["SM2"]["verify"]} == {28, 32, 64}
    assert {len(i["digest"]) // 2 for i in fx["SECP256R1"]["ECGDSA"]["verify"]} == {32, 64}


@pytest.mark.parametrize("curve", S.CURVES)
def test_restatement_gives_the_reference_answers(curve):
    fx = load_fixture()[curve]
    ql = O.qlen(curve)
    for name, alg in S.SCHEMES.items():
        for i in fx[name]["verify"]:
            pub, sig, msg = bytes.fromhex(i["pub"]), bytes.fromhex(i["sig"]), bytes.fromhex(i["msg"])
            dg = bytes.fromhex(i["digest"])
            assert S.verify(curve, alg, pub, sig, dg) == (0 if i["ret"] == 0 else 1), (curve, name, i["family"])
        for i in fx[name]["sign"]:
            x, k = int(i["x"], 16), int(i["k"], 16)
            st, sig = S.sign(curve, alg, x, k, bytes.fromhex(i["digest"]))
            assert st == (0 if i["ret"] == 0 else 1), (curve, name, i["family"], i["ret"])
            assert sig == (bytes.fromhex(i["sig"]) if i["ret"] == 0 else bytes(2 * ql))


def test_fixture_is_what_the_reference_says_now():
    if not O.have_ref():
        pytest.skip("oracle/_ref/libecc_ref.so is not built here")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_sig_family_fixture as M
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
        nw = {8: 8, 12: 12, 17: 17}[(q.bit_length() + 31) // 32]      # the words of q, as the kernels are instantiated
        self.R = 1 << (32 * nw)
        self.consts = (nw, words(q), words(self.R * self.R % q), C.c_uint32((-pow(q, -1, 1 << 32)) % (1 << 32)))
        self.qlen, self.qbits = (q.bit_length() + 7) // 8, q.bit_length()

    def digest_e(self, alg, dg):
        out = (C.c_uint32 * NW)()
        self.lib.t_digest_e(*self.consts, alg, dg, len(dg), self.qlen, self.qbits, out)
        return from_words(out)

    def front_end(self, alg, r, s, dg):
        e = self.digest_e(alg, dg)
        out, div = (C.c_uint32 * (3 * NW))(), (C.c_uint32 * NW)()
        # the divisor first (a call with dinv = 0), then the call with its inverse in Montgomery form
        self.lib.t_front_end(*self.consts, alg, words(r), words(s), words(e), words(0), out, div)
        d = from_words(div)
        dinv = pow(d, -1, self.q) * self.R % self.q if d % self.q and self.lib.t_verify_inverts(alg) else 0
        flag = self.lib.t_front_end(*self.consts, alg, words(r), words(s), words(e), words(dinv), out, div)
        return flag, from_words(out), from_words(out, NW), from_words(out, 2 * NW)

    def sign(self, alg, x, k, dg, wx):
        """(status, r, s) for x, k as loaded"""
        if not self.lib.t_sign_key_ok(*self.consts, alg, words(x)) or not 0 < k < self.q:
            return 1, 0, 0
        xinv = pow(1 + x, -1, self.q) * self.R % self.q if self.lib.t_sign_inverts(alg) else 0
        out = (C.c_uint32 * (2 * NW))()
        st = self.lib.t_sign_rs(*self.consts, alg, words(x), words(k), words(self.digest_e(alg, dg)), words(wx), words(xinv), out)
        return (1, 0, 0) if st else (0, from_words(out), from_words(out, NW))


@pytest.fixture(scope="module")
def shimlib():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "sig_family_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SHIM])
    lib = C.CDLL(so)
    u32p, i = C.POINTER(C.c_uint32), C.c_int
    consts = [i, u32p, u32p, C.c_uint32]
    lib.t_digest_e.argtypes = consts + [i, C.c_char_p, i, i, i, u32p]
    lib.t_front_end.argtypes = consts + [i, u32p, u32p, u32p, u32p, u32p, u32p]
    lib.t_sign_key_ok.argtypes = consts + [i, u32p]
    lib.t_sign_rs.argtypes = consts + [i, u32p, u32p, u32p, u32p, u32p, u32p]
    return lib


def test_scheme_switches(shimlib):
    assert [shimlib.t_alg_known(a) for a in (0, 1, 5, 6, 7, 8, 9)] == [0, 0, 0, 1, 1, 1, 0]
    assert [shimlib.t_verify_inverts(a) for a in (6, 7, 8)] == [1, 1, 0]
    assert [shimlib.t_sign_inverts(a) for a in (6, 7, 8)] == [0, 0, 1]


@pytest.mark.parametrize("curve", S.CURVES)
def test_e_for_every_digest_length(shimlib, curve):
    """digests of 1 .. 128 bytes: random, all ones, zero, and multiples of q (e = 0: ECRDSA's becomes 1) -- on the restatement"""
    q = O.CURVES[curve]["q"]
    sh = Shim(shimlib, q)
    rng = np.random.default_rng(91)
    for hlen in range(1, 129):
        cases = [rng.integers(0, 256, size=hlen, dtype=np.uint8).tobytes(), b"\xff" * hlen, bytes(hlen)]
        if 8 * hlen >= q.bit_length():
            m = ((1 << (8 * hlen)) - 1) // q
            cases += [(q * m).to_bytes(hlen, "big"), (q * m).to_bytes(hlen, "little"), q.to_bytes(hlen, "big"), q.to_bytes(hlen, "little")]
        for dg in cases:
            for alg in S.SCHEMES.values():
                assert sh.digest_e(alg, dg) == S.digest_e(alg, dg, q), (curve, alg, hlen)
    assert sh.digest_e(S.ECRDSA, bytes(32)) == 1 and sh.digest_e(S.SM2, bytes(32)) == 0 and sh.digest_e(S.ECGDSA, bytes(32)) == 0


@pytest.mark.parametrize("curve", S.CURVES)
def test_front_end_on_the_fixture_inputs(shimlib, curve):
    q = O.CURVES[curve]["q"]
    ql = O.qlen(curve)
    sh = Shim(shimlib, q)
    fx = load_fixture()[curve]
    for name, alg in S.SCHEMES.items():
        for i in fx[name]["verify"]:
            sig, dg = bytes.fromhex(i["sig"]), bytes.fromhex(i["digest"])
            r, s = int.from_bytes(sig[:ql], "big"), int.from_bytes(sig[ql:], "big")
            assert sh.front_end(alg, r, s, dg) == S.front_end(alg, q, r, s, dg), (curve, name, i["family"])


@pytest.mark.parametrize("curve", ["SECP256R1", "SECP224K1", "SECP521R1", "WEI25519"])
def test_front_end_where_no_hash_leads(shimlib, curve):
    """e = 0 mod q and the range edges of r and s for every scheme -- on the restatement"""
    q = O.CURVES[curve]["q"]
    sh = Shim(shimlib, q)
    rng = np.random.default_rng(92)
    ql = O.qlen(curve)
    top = (1 << (8 * ql)) - 1
    zero_e = [bytes(32), q.to_bytes(ql, "big") if 8 * ql == q.bit_length() else bytes(ql), (q * 3).to_bytes(ql + 1, "big")]
    for alg in S.SCHEMES.values():
        for dg in zero_e + [rng.integers(0, 256, size=48, dtype=np.uint8).tobytes()]:
            if alg == S.SM2 and dg in zero_e:
                assert S.digest_e(alg, dg, q) == 0
            for r in (0, 1, 2, q - 1, q, min(top, q + 1), top, S.rand_int(rng, q)):
                for s in (0, 1, q - 1, q, top, S.rand_int(rng, q), (q - r) % q):
                    got = sh.front_end(alg, r, s, dg)
                    assert got == S.front_end(alg, q, r, s, dg), (curve, alg, r, s)
                    if r >= q or s >= q or r == 0 or s == 0 or (alg == S.SM2 and (r + s) % q == 0):
                        assert got == (1, 0, 0, 0)
    # SM2 with e = 0: the target is r itself; ECGDSA with e = 0: u = 0; ECRDSA with e = 0 -> 1: u = s, v = -r
    assert sh.front_end(S.SM2, 5, 7, bytes(32)) == (0, 7, 12, 5)
    assert sh.front_end(S.ECGDSA, 5, 7, bytes(32))[1] == 0
    assert sh.front_end(S.ECRDSA, 5, 7, bytes(32)) == (0, 7, q - 5, 5)


@pytest.mark.parametrize("curve", S.CURVES)
def test_signing_back_end(shimlib, curve):
    p, a, b, q, G = S._curve(curve)
    ql = O.qlen(curve)
    sh = Shim(shimlib, q)
    fx = load_fixture()[curve]
    for name, alg in S.SCHEMES.items():
        for i in fx[name]["sign"]:
            x, k, dg = int(i["x"], 16), int(i["k"], 16), bytes.fromhex(i["digest"])
            W = O.py_mul(k % O.CURVES[curve]["order"], G, a, p) if k else None
            st, r, s = sh.sign(alg, x, k, dg, W[0] % q if W else 0)
            assert st == (0 if i["ret"] == 0 else 1), (curve, name, i["family"])
            if st == 0:
                assert r.to_bytes(ql, "big") + s.to_bytes(ql, "big") == bytes.fromhex(i["sig"])
    # where no hash leads (on the restatement): e = 0, and SM2's r + k = q, which the reference does not restart on
    rng = np.random.default_rng(93)
    for alg in S.SCHEMES.values():
        for _ in range(20):
            x, k, wx = 1 + S.rand_int(rng, q - 2), 1 + S.rand_int(rng, q - 1), S.rand_int(rng, q)
            for dg in (bytes(32), rng.integers(0, 256, size=64, dtype=np.uint8).tobytes()):
                rs = S.sign_rs(alg, q, x, k, S.digest_e(alg, dg, q), wx)
                assert sh.sign(alg, x, k, dg, wx) == ((0,) + rs if rs else (1, 0, 0))
    x, k = 1 + S.rand_int(rng, q - 2), 1 + S.rand_int(rng, q - 1)
    st, r, s = sh.sign(S.SM2, x, k, bytes(32), (q - k) % q)     # e = 0, r = wx = q - k
    assert (st, r, s) == (0, q - k, k)                          # s = (k + k x) / (1 + x) = k


def test_header_binding_and_library_have_the_calls():
    with open(os.path.join(ROOT, "include", "libecc_amd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = libecc_amd.load_library()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in libecc_amd.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    for macro, val in (("ECAMD_SIG_ECGDSA", 6), ("ECAMD_SIG_ECRDSA", 7), ("ECAMD_SIG_SM2", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, val), src)
    assert (libecc_amd.api.SIG_ECGDSA, libecc_amd.api.SIG_ECRDSA, libecc_amd.api.SIG_SM2) == (6, 7, 8)
    for m in ("sig_verify", "sig_sign", "sig_verify_dev", "sig_sign_dev"):
        assert hasattr(libecc_amd.api.Curve, m)
