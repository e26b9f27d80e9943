#!/usr/bin/env python3
"""Record the UNMODIFIED reference's answers for HMAC and deterministic ECDSA over the whole hash table, so that this pin travels without
oracle/_ref:
    python tests/golden/make_hmac_ht_fixture.py  ->  tests/golden/hmac_ht.json
"hmac":   per served hash, libecc's hmac() of hmac_ht_ref.msg_bytes(mlen) under hmac_ht_ref.key_bytes(klen) at hmac_ht_ref.hmac_pairs(hash).
"decdsa": per (curve, hash) of hmac_ht_ref.CURVES x hmac_ht_ref.NEW_NAMES, ec_key_pair_import_from_priv_key_buf + _ec_sign with DECDSA and
          no `rand` hook for the items hmac_ht_ref.derive(curve, hash, i), and for the keys 0, q - 1 and q over "sample": the
          reference's return value, whatever it is.
The answers are written compactly (hmac_ht_ref.load_fixture): the first few in full, a four-octet tag per signature, and a SHA-256 over
all of them; the nonces are not recorded (k = s^-1 (e + x r) follows from a signature).
Asserted with the Python restatement, for every hash hashlib has: the solved nonce is the restatement's; at least one brainpoolP256r1
item rejected a candidate; none reached the bound of 1000."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracles as O  # noqa: E402
import hmac_ht_ref as M  # noqa: E402


def build():
    hm = {}
    for name in M.NAMES:
        macs = []
        for kl, ml in M.hmac_pairs(name):
            mac = M.ref_hmac(name, M.key_bytes(kl), M.msg_bytes(ml))
            if M.have_hashlib(name):
                assert mac == M.py_hmac(name, M.key_bytes(kl), M.msg_bytes(ml)), (name, kl, ml)
            macs.append(mac)
        hm[name] = {"first": [m.hex() for m in macs[:M.N_FULL_MACS]], "all": M.checksum(macs)}
    dec = {}
    for curve in M.CURVES:
        for name in M.NEW_NAMES:
            sigs, rejected = [], 0
            for i in range(M.n_items(curve)):
                priv, msg = M.derive(curve, name, i)
                ret, sig = M.ref_sign(curve, name, priv, msg)
                assert ret == 0, (curve, name, i, ret)
                if M.have_hashlib(name):
                    h1 = M.ref_hash(name, msg)
                    assert h1 == M.py_hash(name, msg)
                    pk, retries = M.py_nonce(curve, name, priv, h1)
                    assert pk == M.k_from_sig(curve, priv, h1, sig) and retries < M.MAX_RETRIES, (curve, name, i)
                    rejected += retries
                sigs.append(sig)
            if curve == M.RETRY_CURVE and M.have_hashlib(name):
                assert rejected > 0, (curve, name)
            edges = [M.ref_sign(curve, name, priv, M.EDGE_MSG) for priv in M.edge_keys(curve)]
            assert edges[2][0] == -2, (curve, name, edges)      # x = q must not import
            dec["%s/%s" % (curve, name)] = {"first": [s.hex() for s in sigs[:M.N_FULL_SIGS]], "tags": [M.tag(s) for s in sigs],
                                            "edges": [ret for ret, _ in edges],
                                            "all": M.checksum(sigs + [s for ret, s in edges if ret == 0])}
    return {"hmac": hm, "decdsa": dec}


def dumps(fx):
    """one hash and one (curve, hash) pair per line"""
    out = []
    for part in ("hmac", "decdsa"):
        rows = [json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in fx[part].items()]
        out.append(json.dumps(part) + ": {\n" + ",\n".join(rows) + "\n}")
    return "{\n" + ",\n".join(out) + "\n}\n"


def main():
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    fx = build()
    with open(M.FIXTURE, "w") as f:
        f.write(dumps(fx))
    print("wrote", len(fx["hmac"]), "hashes,", sum(len(v["tags"]) for v in fx["decdsa"].values()), "signatures")


if __name__ == "__main__":
    main()
