"""Writes tests/golden/det_sign.json: what the UNMODIFIED reference (oracle/_ref/libecc_ref.so, through tests/det_sign_ref.py) answers
to ec_key_pair_import_from_priv_key_buf + _ec_sign for DBIGN (no `rand` hook: its own generator runs) and for BIP0340 (the `rand`
hook supplies the aux value), beside the Python restatement's nonce (and, for DBIGN, the candidates it rejected).

  dbign, per curve of det_sign_ref.DBIGN_CURVES and per hash (BELT, SHA-224 / 256 / 384 / 512):
    t         a random key and message with a non-empty and with an empty additional data t
    x_edge    x = 0, 1, q - 1, q under two hashes per curve (det_sign_ref.dbign_edge_hashes: every hash on some curve): the
              reference's return value is recorded, whatever it is
    retry0 / retry1 / retry2   on the two curves whose order rejects candidates: found by search, items whose generator rejects
              none, exactly one and at least two candidates
  bip0340, per curve of det_sign_ref.BIP_CURVES and per hash:
    edge      messages that put the NONCE hash's input length on each of schnorr_ref.PAD_EDGES modulo the hash's block
  and under two hashes per curve (det_sign_ref.bip_edge_hashes: every hash on some curve):
    aux       aux = 0, all-ones, random
    x_edge    x = 0, 1, q - 1, q
    parity    a key with an odd and one with an even Y.y
  dbign_vectors / bip0340_vectors   the reference's own signing vectors (src/tests/dbign_test_vectors.h 1-3: dbign256v1 with
              belt-hash; src/tests/bip0340_test_vectors.h), read as data where the reference tree is present and otherwise kept from
              the file already written
Every item with ret = 0 must carry the signature the restatement computes from its own nonce; the script asserts it, and that each
family holds both outcomes where both are possible.  Run from the repository root:  python tests/golden/make_det_sign_fixture.py"""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracles as O          # noqa: E402
import sigfam_ref as R       # noqa: E402
import bign_ref as B         # noqa: E402
import schnorr_ref as S      # noqa: E402
import det_sign_ref as D     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "det_sign.json")
REF_TESTS = "/root/reference/src/tests"


def dbign_item(curve, h, family, x, oid, t, msg):
    ql = O.qlen(curve)
    ret, sig = D.ref_dbign_sign(curve, h, oid, t, x, msg)
    (st, mine), (k, rej) = D.dbign_sign(curve, h, x, oid, t, msg)
    assert (ret == 0) == (st == 0) and (ret != 0 or sig == mine), (curve, h, family)
    return {"family": family, "hash": h, "oid": oid.hex(), "t": t.hex(), "msg": msg.hex(), "x": x.to_bytes(ql, "big").hex(), "ret": ret,
            "sig": sig.hex() if sig else None, "k": k.to_bytes(ql, "big").hex(), "rejects": rej}


def bip_item(curve, h, family, x, aux, msg):
    ql = O.qlen(curve)
    ret, sig = S.ref_sign(curve, S.BIP0340, h, x, aux, msg)
    (st, mine), k = D.bip_sign(curve, h, x, aux, msg)
    assert (ret == 0) == (st == 0) and (ret != 0 or sig == mine), (curve, h, family)
    pub = D.bip_pub(curve, x) if 0 < x < O.CURVES[curve]["q"] else None
    return {"family": family, "hash": h, "msg": msg.hex(), "x": x.to_bytes(ql, "big").hex(), "aux": aux.to_bytes(ql, "big").hex(), "ret": ret,
            "sig": sig.hex() if sig else None, "k": k.to_bytes(ql, "big").hex(), "y_odd": None if pub is None else pub[-1] & 1}


def c_bytes(text, name):
    m = re.search(r"%s\[\]\s*=\s*\{(.*?)\};" % re.escape(name), text, re.S)
    return bytes(int(v, 16) for v in re.findall(r"0x([0-9a-fA-F]{2})", m.group(1)))


def c_msg(text, case):
    m = re.search(r"%s_test_case = \{.*?\.msg = \"(.*?)\",\s*\.msglen = (\d+)" % case, text, re.S)
    msg = bytes(int(v, 16) for v in re.findall(r"\\x([0-9a-fA-F]{2})", m.group(1)))
    assert len(msg) == int(m.group(2))
    return msg


def reference_vectors():
    """the reference's own vectors, as data; None where its tree is not here"""
    if not os.path.isdir(REF_TESTS):
        return None
    dv, bv = [], []
    text = open(os.path.join(REF_TESTS, "dbign_test_vectors.h")).read()
    for j in (1, 2, 3):
        ad = c_bytes(text, "dbign_%d_test_vectors_adata" % j)
        ol, tl = int.from_bytes(ad[:2], "big"), int.from_bytes(ad[2:4], "big")
        dv.append({"curve": "BIGN256V1", "hash": "BELT", "x": c_bytes(text, "dbign_%d_test_vectors_priv_key" % j).hex(),
                   "oid": ad[4:4 + ol].hex(), "t": ad[4 + ol:4 + ol + tl].hex(), "msg": c_msg(text, "dbign_%d" % j).hex(),
                   "sig": c_bytes(text, "dbign_%d_test_vectors_expected_sig" % j).hex()})
    text = open(os.path.join(REF_TESTS, "bip0340_test_vectors.h")).read()
    for j in (1, 2, 3, 4):
        fn = re.search(r"bip0340_%d_nn_random_test_vector\(.*?k_buf\[\]\s*=\s*\{(.*?)\};" % j, text, re.S)
        aux = bytes(int(v, 16) for v in re.findall(r"0x([0-9a-fA-F]{2})", fn.group(1)))
        bv.append({"curve": "SECP256K1", "hash": "SHA256", "x": c_bytes(text, "bip0340_%d_test_vectors_priv_key" % j).hex(), "aux": aux.hex(),
                   "msg": c_msg(text, "bip0340_%d" % j).hex(), "sig": c_bytes(text, "bip0340_%d_test_vectors_expected_sig" % j).hex()})
    return dv, bv


def build():
    out = {"dbign": {}, "bip0340": {}}
    for ci, curve in enumerate(D.DBIGN_CURVES):
        q, ql = O.CURVES[curve]["q"], O.qlen(curve)
        rng = np.random.default_rng(3410145 + ci)
        items = []
        for h in D.DBIGN_HASHES:
            x, msg = 1 + R.rand_int(rng, q - 1), rng.integers(0, 256, size=20, dtype=np.uint8).tobytes()
            items.append(dbign_item(curve, h, "t", x, B.OID_BELT, D.T_SAMPLE, msg))
            items.append(dbign_item(curve, h, "t", x, B.OID_BELT, b"", msg))
            for xe in (0, 1, q - 1, q) if h in D.dbign_edge_hashes(curve) else ():
                items.append(dbign_item(curve, h, "x_edge", xe, B.OID_BELT, b"", b"sample"))
            if curve in D.RETRY_CURVES:
                want = {"retry0": 1, "retry1": 1, "retry2": 1}
                while any(want.values()):
                    x, msg = 1 + R.rand_int(rng, q - 1), rng.integers(0, 256, size=16, dtype=np.uint8).tobytes()
                    rej = D.dbign_nonce(curve, h, x, B.OID_BELT, b"", msg)[2]
                    fam = "retry%d" % min(rej, 2)
                    if want[fam]:
                        want[fam] -= 1
                        items.append(dbign_item(curve, h, fam, x, B.OID_BELT, b"", msg))
            edge = {int(i["x"], 16): i["ret"] for i in items if i["hash"] == h and i["family"] == "x_edge"}
            assert not edge or (set(edge.values()) == {0, -2} and edge[0] == 0 and edge[q] == -2), (curve, h, edge)
        out["dbign"][curve] = items
    for ci, curve in enumerate(D.BIP_CURVES):
        q, ql = O.CURVES[curve]["q"], O.qlen(curve)
        rng = np.random.default_rng(340 + ci)
        items = []
        for h in D.BIP_HASHES:
            block = 64 if D.HSIZE[h] <= 32 else 128
            x, aux = 1 + R.rand_int(rng, q - 1), R.rand_int(rng, 1 << (8 * ql))
            for e in S.PAD_EDGES:
                if e < block:
                    n = (e - D.nonce_input_len(curve, h, 0)) % block
                    items.append(bip_item(curve, h, "edge", x, aux, S.pattern_msg(n)))
            if h not in D.bip_edge_hashes(curve):
                continue
            msg = rng.integers(0, 256, size=24, dtype=np.uint8).tobytes()
            for aux in (0, (1 << (8 * ql)) - 1, R.rand_int(rng, 1 << (8 * ql))):
                items.append(bip_item(curve, h, "aux", x, aux, msg))
            for xe in (0, 1, q - 1, q):
                items.append(bip_item(curve, h, "x_edge", xe, aux, msg))
            want = {0, 1}
            while want:
                x = 1 + R.rand_int(rng, q - 1)
                odd = D.bip_pub(curve, x)[-1] & 1
                if odd in want:
                    want.discard(odd)
                    items.append(bip_item(curve, h, "parity", x, R.rand_int(rng, 1 << (8 * ql)), msg))
            mine = [i for i in items if i["hash"] == h]
            edge = {int(i["x"], 16): i["ret"] for i in mine if i["family"] == "x_edge"}
            assert (edge[1] == 0 and edge[q - 1] == 0 and edge[0] != 0 and edge[q] != 0), (curve, h, edge)   # x = 0 and x = q are refused
            assert all(i["ret"] == 0 for i in mine if i["family"] != "x_edge")
            assert {i["y_odd"] for i in mine if i["family"] == "parity"} == {0, 1}
        out["bip0340"][curve] = items
    vec = reference_vectors()
    if vec is None:
        with open(OUT) as f:
            old = json.load(f)
        vec = old["dbign_vectors"], old["bip0340_vectors"]
    out["dbign_vectors"], out["bip0340_vectors"] = vec
    return out


def packed(items):
    """the file's form of a curve's items (det_sign_ref.unpack puts back what is left out): a field of DELTA that the item before has
    too, a ret of 0, a missing signature, a zero nonce, no rejects, an unknown parity; a pattern message goes by its length"""
    out = []
    for j, i in enumerate(items):
        d = {k: v for k, v in i.items() if not (k in D.DELTA and j and items[j - 1].get(k) == v)}
        if "msg" in d and d["msg"] and bytes.fromhex(d["msg"]) == S.pattern_msg(len(d["msg"]) // 2):
            d["msgpat"] = len(d.pop("msg")) // 2
        for k, v in (("ret", 0), ("sig", None), ("k", "00" * (len(i["x"]) // 2)), ("rejects", 0), ("y_odd", None)):
            if k in d and d[k] == v:
                del d[k]
        out.append(d)
    return out


def dumps(fx):
    js = lambda v: json.dumps(v, separators=(",", ":"))
    parts = []
    for kind in ("dbign", "bip0340"):
        parts.append(js(kind) + ": {\n" + ",\n".join(js(c) + ": [\n" + ",\n".join(js(i) for i in packed(items)) + "\n]"
                                                     for c, items in fx[kind].items()) + "\n}")
    for kind in ("dbign_vectors", "bip0340_vectors"):
        parts.append(js(kind) + ": [\n" + ",\n".join(js(i) for i in fx[kind]) + "\n]")
    return "{\n" + ",\n".join(parts) + "\n}\n"


if __name__ == "__main__":
    text = dumps(build())
    with open(OUT, "w") as f:
        f.write(text)
