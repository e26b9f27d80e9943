#!/usr/bin/env python3
"""Record the UNMODIFIED reference's answers for ECKCDSA, ECSDSA, ECOSDSA, ECFSDSA and BIP0340 under every hash of ec_digest_slots_batch
that the older entry points refuse, so that this pin travels without oracle/_ref:
    python tests/golden/make_sighash_ht_fixture.py  ->  tests/golden/sighash_ht.json
Per case (scheme, curve, hash) of sighash_ht_ref.cases() x sighash_ht_ref.NEW_NAMES: ec_key_pair_import_from_priv_key_buf + _ec_sign with
the `rand` hook returning the item's nonce (BIP0340: its aux value) for the 130 signing items, and ec_pub_key_import_from_aff_buf +
ec_verify for the 130 verification items built from those signatures (sighash_ht_ref.sign_item / verify_item).  The answers are
written compactly (sighash_ht_ref.pack / load_fixture): a one-character tag per signature, a SHA-256 over all of them, the verdicts of the
corrupted items as a string, and the first signatures in full for three or four hashes per (scheme, curve), every hash on one curve of every scheme.
Asserted while recording: the reference signs every item outside SIGN_EDGES and accepts every signature that was not corrupted, so
no test has a reason to skip an item.  For BIP0340 the parity of every commitment is recorded from a Python multiplication, and every
combination of the parities of Y.y and R.y is asserted to occur in every case."""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracles as O  # noqa: E402
import sighash_ht_ref as R  # noqa: E402


def record(args):
    scheme, curve, name = args
    alg = R.SCHEMES[scheme]
    p, a, b, q, G = R._curve(curve)
    sigs, rets, rodd = [], [], []
    for i in range(R.N):
        x, v, msg = R.sign_item(scheme, curve, name, i)
        ret, sig = R.ref_sign(scheme, curve, name, x, v, msg)
        if i in R.SIGN_EDGES:
            rets.append(ret)
        else:
            assert ret == 0, (scheme, curve, name, i, ret)
        sigs.append(sig)
        if alg == R.BIP0340:
            if sig is None:
                rodd.append("-")
            else:
                ke = R.bip_k_even(name, curve, i % R.N_KEYS, sig, msg)
                W = R.py_mul(ke, G, a, p)                       # [k']G has an even y; R.y of the generator's k is odd iff k != k'
                assert W[0] == int.from_bytes(sig[:O.clen(curve)], "big") and not W[1] & 1, (curve, name, i)
                k = R.py_bip_nonce(name, curve, x, v, msg)
                assert k in (ke, q - ke), (curve, name, i)
                rodd.append("1" if k != ke else "0")
    ver = []
    for i in range(R.N):
        pk, sig, msg, fault = R.verify_item(scheme, curve, name, i, sigs)
        if fault:
            ver.append("1")
            continue
        v = R.ref_verify(scheme, curve, name, pk, sig, msg)
        if i not in R.VERIFY_EDGES or (alg == R.ECKCDSA and R.VERIFY_EDGES[i].startswith("slot_")):
            assert v == 0, (scheme, curve, name, i)
        ver.append(str(v))
    if alg == R.BIP0340:
        combos = {(i % R.N_KEYS < 4, rodd[i]) for i in range(R.N) if rodd[i] != "-"}
        assert combos == {(True, "0"), (True, "1"), (False, "0"), (False, "1")}, (curve, name, combos)
    signed = [s for s in sigs if s is not None]
    rec = {"first": [s.hex() for s in sigs[:R.N_FULL]] if R.full_kept(scheme, curve, name) else [], "tags": "".join(R.tag(s) for s in signed),
           "rets": rets, "all": R.checksum(signed), "ver": "".join(ver)}
    if alg == R.BIP0340:
        rec["rodd"] = "".join(rodd)
    return R.case_key(scheme, curve, name), R.pack(rec)


def main():
    assert O.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    R.M.shim()                                                  # built once, before the workers start
    jobs = [(s, c, n) for s, c in R.cases() for n in R.NEW_NAMES]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        out = dict(ex.map(record, jobs, chunksize=2))
    with open(R.FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main()
