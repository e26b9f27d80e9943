#!/usr/bin/env python3
"""Record the UNMODIFIED reference's answers for EdDSA from messages of any length, so that this pin travels without oracle/_ref:
    python tests/golden/make_eddsa_msgs_fixture.py  ->  tests/golden/eddsa_msgs.json
Per variant (EDDSA25519 / CTX / PH, EDDSA448 / PH) and per case of eddsa_msgs_ref.cases(alg) -- contexts of 0, 1 and 255 octets where the
variant takes one; messages of 0, 1, 7, 8, 9, 15, 16, 17 octets, the lengths that put the hashes that absorb the message at the edges
of a SHA-512 block (111 / 112 / 113, 127 / 128 / 129 and one block further) or of SHAKE256's rate (135 / 136 / 137, 271 / 272 / 273),
4093 octets (just past the longest slot) and 70 001 octets -- the reference's public key (eddsa_import_key_pair_from_priv_key_buf +
eddsa_export_pub_key), its signature (_ec_sign) and its verdicts (eddsa_import_pub_key + ec_verify) on the honest triple, on a flipped
bit in R, in S, in A and in the last message octet (not for the empty message), on S + q and under the next case's key.
The inputs are generated from seeds (eddsa_msgs_ref.case_input); only answers are written.
Asserted here: every edge is reached by r_hash's and hram's input (the pre-hash's for the PH variants); the honest verdict is 0 and every
other one -1; the Python restatement eddsa_sign_ref.py_sign gives the reference's key and signature."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracles as O  # noqa: E402
import eddsa_sign_ref as E  # noqa: E402
import eddsa_msgs_ref as D  # noqa: E402


def build():
    out, parts = {}, []
    for name, alg in zip(D.NAMES, D.ALGS):
        cov = D.coverage(alg)
        assert cov and all(v == set(D.edges(alg)) for v in cov.values()), (name, cov)
        assert set(cov) == ({"prehash"} if E.is_ph(alg) else {"r_hash", "hram"})
        n = len(D.cases(alg))
        pubs, sigs = [], []
        for idx in range(n):
            sk, adata, msg = D.case_input(alg, idx)
            ret, pub, sig = E.ref_sign(alg, sk, adata, msg)
            assert ret == 0, (name, idx, ret)
            assert E.py_sign(alg, sk, adata if adata is not None else b"", msg) == (pub, sig), (name, idx)
            pubs.append(pub)
            sigs.append(sig)
        verdicts = []
        for idx in range(n):
            sk, adata, msg = D.case_input(alg, idx)
            var = D.damaged(alg, pubs[idx], sigs[idx], msg, pubs[(idx + 1) % n])
            v = [D.ref_verify(alg, p, s, adata, m) for _, p, s, m in var]
            assert [k for k, _, _, _ in var] == [k for k in D.KINDS if msg or k != "msg"]
            assert v == [0] + [-1] * (len(var) - 1), (name, idx, v)
            verdicts.append(",".join(str(x) for x in v))
        out[name] = {"pubs": [p.hex() for p in pubs], "sigs": [s.hex() for s in sigs], "verdicts": verdicts}
        parts += pubs + sigs
    return {"cases": out, "sha256": hashlib.sha256(b"".join(parts)).hexdigest()}


def dumps(fx):
    """one list per line"""
    rows = []
    for name, rec in fx["cases"].items():
        body = ",\n".join("  " + json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in rec.items())
        rows.append(json.dumps(name) + ": {\n" + body + "\n}")
    return '{\n"cases": {\n' + ",\n".join(rows) + '\n},\n"sha256": ' + json.dumps(fx["sha256"]) + "\n}\n"


def main():
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    fx = build()
    with open(D.FIXTURE, "w") as f:
        f.write(dumps(fx))
    print("wrote", sum(len(v["sigs"]) for v in fx["cases"].values()), "cases,", os.path.getsize(D.FIXTURE), "octets")


if __name__ == "__main__":
    main()
