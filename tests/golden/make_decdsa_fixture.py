"""Writes tests/golden/decdsa.json: what the UNMODIFIED reference (oracle/_ref/libecc_ref.so, through tests/decdsa_ref.py) answers
to ec_key_pair_import_from_priv_key_buf + _ec_sign with DECDSA and no `rand` hook, beside the Python restatement's nonce and the
number of candidates it rejected.  Per curve of decdsa_ref.CURVES and per hash:
  msg_len   messages of 0, 1, 55, 56, 64, 111, 112, 200 bytes under random keys
  x_edge    x = 0, 1, q - 1, q, 2^(8 qlen) - 1: the reference's return value is recorded, whatever it is
  retry1 / retry2   on the three curves whose order rejects candidates: found by search, items whose generator rejects exactly one and
            at least two candidates (the msg_len items supply the ones with none)
Run from the repository root:  python tests/golden/make_decdsa_fixture.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracles as O          # noqa: E402
import decdsa_ref as D       # noqa: E402
import sigfam_ref as R       # noqa: E402


def item(curve, h, family, x, msg):
    ql = O.qlen(curve)
    priv = x.to_bytes(ql, "big")
    ret, sig = D.ref_sign(curve, h, priv, msg)
    k, retries = D.nonce(curve, h, priv, msg)
    return {"family": family, "hash": h, "msg": msg.hex(), "x": priv.hex(), "ret": ret, "sig": sig.hex() if sig else None,
            "k": k.to_bytes(ql, "big").hex(), "retries": retries}


def build():
    out = {}
    for ci, curve in enumerate(D.CURVES):
        q, ql = O.CURVES[curve]["q"], O.qlen(curve)
        rng = np.random.default_rng(6979 + ci)
        items = []
        for h in D.HASHES:
            for n in D.MSG_LENS:
                items.append(item(curve, h, "msg_len", 1 + R.rand_int(rng, q - 1), rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()))
            for x in (0, 1, q - 1, q, (1 << (8 * ql)) - 1):
                items.append(item(curve, h, "x_edge", x, b"sample"))
            if curve in D.RETRY_CURVES:
                want = {"retry1": 2, "retry2": 2}
                while any(want.values()):
                    x, msg = 1 + R.rand_int(rng, q - 1), rng.integers(0, 256, size=16, dtype=np.uint8).tobytes()
                    r = D.nonce(curve, h, x.to_bytes(ql, "big"), msg)[1]
                    fam = "retry1" if r == 1 else "retry2" if r >= 2 else None
                    if fam and want[fam]:
                        want[fam] -= 1
                        items.append(item(curve, h, fam, x, msg))
        out[curve] = items
    return out


def dumps(fx):
    return "{\n" + ",\n".join(json.dumps(c) + ": [\n" + ",\n".join(json.dumps(i) for i in items) + "\n]" for c, items in fx.items()) + "\n}\n"


if __name__ == "__main__":
    with open(os.path.join(ROOT, "tests", "golden", "decdsa.json"), "w") as f:
        f.write(dumps(build()))
