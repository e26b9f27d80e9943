#!/usr/bin/env python3
"""Record the UNMODIFIED reference's answers for the ragged message array, so that this pin travels without oracle/_ref:
    python tests/golden/make_digest_msgs_fixture.py  ->  tests/golden/digest_msgs.json
"digests": per served hash, the reference's one-shot hash of call prefix || item prefix || message for digest_msgs_ref.cases(hash): the
           totals around every block and length-field boundary, 4092 / 4093 / 4097 (the longest slot and just past it) and 70 001 octets,
           each split four ways over the three segments.
"proto":   per (curve, hash) of digest_msgs_ref.PROTO, for six messages of 0 .. 70 001 octets: the reference's DECDSA signature
           (ec_key_pair_import_from_priv_key_buf + _ec_sign, no `rand` hook) and its ECDSA verdicts (ec_pub_key_import_from_aff_buf +
           ec_verify) on that signature, on the signature with a flipped bit, and on the message with a flipped bit in its last octet.
The inputs are generated from seeds (digest_msgs_ref.case_input, proto_item); only answers are written: variant 0 of every total in
full, an 8-octet tag per case, and SHA-256 sums.
Asserted here: the splits reach every residue mod 4 of every segment length for every hash; all three segments are empty once; hashlib
agrees where it has the hash; the verdicts are [0, -1, -1] for every message."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracles as O  # noqa: E402
import hmac_ht_ref as M  # noqa: E402
import digest_msgs_ref as D  # noqa: E402


def build():
    digs = {}
    for name in D.NAMES:
        assert D.coverage(name) == ({0, 1, 2, 3},) * 3, (name, D.coverage(name))
        assert D.cases(name)[0] == (0, 0, 0)
        out = []
        for idx in range(len(D.cases(name))):
            x = b"".join(D.case_input(name, idx))
            d = M.ref_hash(name, x)
            if M.have_hashlib(name):
                assert d == M.py_hash(name, x), (name, idx)
            out.append(d)
        digs[name] = {"full": [out[D.VARIANTS * k].hex() for k in range(len(D.totals(name)))], "tags": [D.tag(d) for d in out],
                      "all": D.checksum(out)}
    proto = {}
    for curve, name in D.PROTO:
        sigs, verdicts = [], []
        for i in range(len(D.PROTO_LENS)):
            priv, pub, msg = D.proto_item(curve, name, i)
            ret, sig = M.ref_sign(curve, name, priv, msg)
            assert ret == 0, (curve, name, i, ret)
            v = [D.ref_verify(curve, name, pub, sig, msg), D.ref_verify(curve, name, pub, D.flip_sig(sig), msg),
                 D.ref_verify(curve, name, pub, sig, D.flip_msg(msg))]
            assert v == [0, -1, -1], (curve, name, i, v)
            sigs.append(sig)
            verdicts.append(v)
        proto["%s/%s" % (curve, name)] = {"sigs": [s.hex() for s in sigs], "verdicts": verdicts}
    total = D.checksum([bytes.fromhex(digs[n]["all"]) for n in D.NAMES] + [bytes.fromhex(s) for k in proto for s in proto[k]["sigs"]])
    return {"digests": digs, "proto": proto, "sha256": total}


def dumps(fx):
    """one hash and one (curve, hash) pair per line"""
    out = []
    for part in ("digests", "proto"):
        rows = [json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in fx[part].items()]
        out.append(json.dumps(part) + ": {\n" + ",\n".join(rows) + "\n}")
    out.append('"sha256": ' + json.dumps(fx["sha256"]))
    return "{\n" + ",\n".join(out) + "\n}\n"


def main():
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    fx = build()
    with open(D.FIXTURE, "w") as f:
        f.write(dumps(fx))
    print("wrote", sum(len(v["tags"]) for v in fx["digests"].values()), "digests,", sum(len(v["sigs"]) for v in fx["proto"].values()), "signatures")


if __name__ == "__main__":
    main()
