"""CPU tests of tests/golden/sig_kats.json, the reference's own known answers of ECKCDSA, ECSDSA, ECOSDSA, ECFSDSA, ECGDSA, BIGN and
DBIGN (tests/sigkats_ref.py describes a case; tests/test_gpu_sig_kats.py runs them on the device):
  * the number of cases per family is what the generator printed -- 10 / 8 / 8 / 8 / 4 / 8 / 4, every ec_test_case of these families that
    src/tests/ec_self_tests_core.h, bign_test_vectors.h and dbign_test_vectors.h hold (DBIGN 1 - 3 are in det_sign.json) -- and the
    (family, curve, hash) shapes are pinned, those no other family fixture reaches by name;
  * the Python restatement of each family signs every case to the published bytes and gives every variant's recorded verdict;
  * every case has an accepted and at least three rejected variants, all damaged ones rejected;
  * where oracle/_ref is built the unmodified reference does the same, and where its tree is present the generator reproduces the
    file byte for byte."""
import os
import sys
from collections import Counter

import pytest

import oracles as O
import sigkats_ref as K

hx = bytes.fromhex
COUNTS = {"ECKCDSA": 10, "ECSDSA": 8, "ECOSDSA": 8, "ECFSDSA": 8, "ECGDSA": 4, "BIGN": 8, "DBIGN": 4}
SCHNORR_SHAPES = {("SECP224R1", "SHA224"), ("SECP256R1", "SHA256"), ("SECP384R1", "SHA384"), ("SECP521R1", "SHA512"),
                  ("BRAINPOOLP256R1", "SHA256"), ("BRAINPOOLP384R1", "SHA384"), ("BRAINPOOLP512R1", "SHA512"), ("FRP256V1", "SHA256")}
SHAPES = {
    # SHA-256 on the 224-bit order is the reference's "specific for truncation test"; SHA-512 on secp256r1 has r_len = qlen < hsize
    "ECKCDSA": SCHNORR_SHAPES | {("SECP224R1", "SHA256"), ("SECP256R1", "SHA512")},
    "ECSDSA": SCHNORR_SHAPES,
    "ECOSDSA": SCHNORR_SHAPES,
    "ECFSDSA": SCHNORR_SHAPES,
    "ECGDSA": {("BRAINPOOLP192R1", "SHA256"), ("BRAINPOOLP224R1", "SHA224"), ("BRAINPOOLP256R1", "SHA256"), ("BRAINPOOLP384R1", "SHA384")},
    "BIGN": {("BIGN256V1", "BELT"), ("BIGN384V1", "BASH384"), ("BIGN512V1", "BASH512")},
    "DBIGN": {("BIGN384V1", "BASH384"), ("BIGN512V1", "BASH512")},
}

CASES = K.load_fixture()
IDS = [c["id"] for c in CASES]


def test_counts_and_shapes():
    assert dict(Counter(c["alg"] for c in CASES)) == COUNTS and list(COUNTS) == list(K.ALGS)
    assert len(set(IDS)) == len(CASES) == 50
    assert [c["alg"] for c in CASES] == sorted((c["alg"] for c in CASES), key=list(K.ALGS).index)
    got = {}
    for c in CASES:
        got.setdefault(c["alg"], set()).add((c["curve"], c["hash"]))
    assert got == SHAPES
    curves = {c["curve"] for c in CASES}
    assert {"SECP224R1", "BRAINPOOLP192R1", "BRAINPOOLP224R1", "BRAINPOOLP384R1", "BRAINPOOLP512R1", "FRP256V1", "BIGN384V1",
            "BIGN512V1"} <= curves
    # two 64-octet and two block-straddling BASH messages, and BIGN's and DBIGN's BASH cases on both STB curves
    assert Counter((c["alg"], c["curve"]) for c in CASES if c["hash"].startswith("BASH")) == \
        {("BIGN", "BIGN384V1"): 2, ("BIGN", "BIGN512V1"): 2, ("DBIGN", "BIGN384V1"): 2, ("DBIGN", "BIGN512V1"): 2}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fields_and_variants(case):
    curve, alg, hname = case["curve"], case["alg"], case["hash"]
    ql, cl = O.qlen(curve), O.clen(curve)
    q = O.CURVES[curve]["q"]
    r_len, s_len = K.components(curve, alg, hname)
    assert len(hx(case["sig"])) == r_len + s_len and len(hx(case["pub"])) == 2 * cl
    assert len(hx(case["x"])) == len(hx(case["k"])) == ql
    assert 0 < int(case["x"], 16) < q and 0 < int(case["k"], 16) < q
    assert len(hx(case["digest"])) == K.HSIZE[hname] and hx(case["msg"])
    assert (case["adata"] != "") == (alg in K.BIGNS)
    if alg in K.BIGNS:
        assert len(K.oid_of(case)) == 11
    vs = case["variants"]
    assert len(vs) in (4, 5) and [v["ret"] for v in vs] == [0] + [-1] * (len(vs) - 1)
    honest = (case["pub"], case["sig"], case["msg"])
    assert (vs[0]["pub"], vs[0]["sig"], vs[0]["msg"]) == honest
    # each damaged variant differs from the honest triple in one field, and there by one bit (the foreign key: a whole other key)
    sig, msg = hx(case["sig"]), hx(case["msg"])

    def bits(a, b):
        return len(a) == len(b) and sum(bin(u ^ v).count("1") for u, v in zip(a, b))

    for j, field in ((1, "sig"), (2, "sig"), (3, "msg"), (4, "pub")):
        if j < len(vs):
            assert [f for f in ("pub", "sig", "msg") if vs[j][f] != case[f]] == [field], (case["id"], j)
    d1 = [i for i, (u, v) in enumerate(zip(sig, hx(vs[1]["sig"]))) if u != v]
    d2 = [i for i, (u, v) in enumerate(zip(sig, hx(vs[2]["sig"]))) if u != v]
    assert bits(sig, hx(vs[1]["sig"])) == 1 and bits(sig, hx(vs[2]["sig"])) == 1 and d1[0] < r_len <= d2[0]
    assert bits(msg, hx(vs[3]["msg"])) == 1 and msg[0] ^ hx(vs[3]["msg"])[0] == 0x80
    if len(vs) == 5:
        assert len(hx(vs[4]["pub"])) == 2 * cl and any(c["pub"] == vs[4]["pub"] and c["curve"] == curve for c in CASES)
    else:
        assert all(c["pub"] == case["pub"] for c in CASES if c["curve"] == curve)      # no other key on this curve


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_python_restatement(case):
    curve, alg, hname = case["curve"], case["alg"], case["hash"]
    x, k, msg, sig = int(case["x"], 16), int(case["k"], 16), hx(case["msg"]), hx(case["sig"])
    oid = K.oid_of(case) if alg in K.BIGNS else b""
    dg = K.py_digest(hname, msg)
    assert dg == hx(case["digest"])
    assert K.pub_of(curve, alg, x) == hx(case["pub"])
    if alg == "DBIGN":
        assert K.k_from_sig(curve, x, dg, sig) == k
    assert K.py_sign(curve, alg, hname, x, k, msg, dg, oid) == (0, sig)
    for j, v in enumerate(case["variants"]):
        vm = hx(v["msg"])
        got = K.py_verify(curve, alg, hname, hx(v["pub"]), hx(v["sig"]), vm, K.py_digest(hname, vm), oid)
        assert got == (0 if v["ret"] == 0 else 1), (case["id"], j)


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref is not built")
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference(case):
    curve, alg, hname = case["curve"], case["alg"], case["hash"]
    x, k, msg, sig = int(case["x"], 16), int(case["k"], 16), hx(case["msg"]), hx(case["sig"])
    oid = K.oid_of(case) if alg in K.BIGNS else b""
    assert K.ref_digest(hname, msg) == hx(case["digest"])
    assert K.ref_sign(curve, alg, hname, x, k, msg, oid) == (0, sig)
    if alg == "DBIGN":
        assert K.ref_dbign_sign(curve, hname, x, msg, oid) == (0, sig)
    for j, v in enumerate(case["variants"]):
        assert K.ref_verify(curve, alg, hname, hx(v["pub"]), hx(v["sig"]), hx(v["msg"]), oid) == v["ret"], (case["id"], j)


def test_regenerating_gives_the_same_file():
    sys.path.insert(0, os.path.join(O.GOLDEN))
    try:
        import extract_kats as E
        if not (O.have_ref() and os.path.exists(os.path.join(E.REF, "ec_self_tests_core.h"))):
            pytest.skip("the reference tree or oracle/_ref is not here")
        import make_sig_kats_fixture as G
        with open(K.FIXTURE) as f:
            assert G.dumps(G.build()) == f.read()
    finally:
        sys.path.remove(O.GOLDEN)
