"""GPU tests of batched BIGN / DBIGN (ec_bign_verify_batch / ec_bign_sign_batch and their _dev forms) against the recorded answers of
the unmodified reference (tests/golden/bign.json), the Python restatement of tests/bign_ref.py, and, where oracle/_ref is built, the
reference itself."""
import ctypes as C

import numpy as np
import pytest

import libecc_amd
from libecc_amd import api as A
import oracles as O
import bign_ref as B
import sighash_ref as S

pytestmark = pytest.mark.gpu
HT = {"SHA224": 1, "SHA256": 2, "SHA384": 3, "SHA512": 4, "BELT": 16}


@pytest.fixture(scope="module")
def ctx():
    c = libecc_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    import os
    return B.load_fixture(os.path.join(O.GOLDEN, "bign.json"))


def be(v, n):
    return v.to_bytes(n, "big")


def run_verify(cv, items, slots, alg=A.SIG_BIGN):
    """the items grouped by (hash, OID): one call per group; slots: message slots hashed on the device, else digests"""
    out = [None] * len(items)
    groups = {}
    for j, i in enumerate(items):
        groups.setdefault((i["hash"], i["oid"]), []).append(j)
    for (h, oid), idx in groups.items():
        msgs = [bytes.fromhex(items[j]["msg"]) for j in idx]
        stride = B.stride_for(max(len(m) for m in msgs)) if slots else B.HSIZE[h]
        inp = b"".join(B.device_input(h, m, stride if slots else None) for m in msgs)
        res = cv.bign_verify(alg, HT[h] if slots else 0, b"".join(bytes.fromhex(items[j]["pub"]) for j in idx),
                             b"".join(bytes.fromhex(items[j]["sig"]) for j in idx), inp, stride, bytes.fromhex(oid))
        for j, r in zip(idx, res):
            out[j] = r
    return out


def run_sign(cv, items, slots, ql, alg=A.SIG_BIGN):
    out = [None] * len(items)
    groups = {}
    for j, i in enumerate(items):
        groups.setdefault((i["hash"], i["oid"]), []).append(j)
    sl = ql // 2 + ql
    for (h, oid), idx in groups.items():
        msgs = [bytes.fromhex(items[j]["msg"]) for j in idx]
        stride = B.stride_for(max(len(m) for m in msgs)) if slots else B.HSIZE[h]
        inp = b"".join(B.device_input(h, m, stride if slots else None) for m in msgs)
        sigs, st = cv.bign_sign(alg, HT[h] if slots else 0, b"".join(bytes.fromhex(items[j]["x"])[-ql:] for j in idx),
                                b"".join(bytes.fromhex(items[j]["k"])[-ql:] for j in idx), inp, stride, bytes.fromhex(oid))
        for n, j in enumerate(idx):
            out[j] = (st[n], sigs[n * sl:(n + 1) * sl])
    return out


def check_fixture(cv, d, curve, slots, alg=A.SIG_BIGN):
    ql = O.qlen(curve)
    got = run_verify(cv, d["verify"], slots, alg)
    for i, g in zip(d["verify"], got):
        assert g == (0 if i["ret"] == 0 else 1), (curve, i["family"], i["hash"], slots)
    # x = q does not fit the reference's import (-2); the call takes qlen bytes, where q fits: status 1
    got = run_sign(cv, d["sign"], slots, ql, alg)
    for i, (st, sig) in zip(d["sign"], got):
        assert st == (0 if i["ret"] == 0 else 1), (curve, i["family"], slots)
        assert sig == (bytes.fromhex(i["out"]) if i["ret"] == 0 else bytes(ql // 2 + ql)), (curve, i["family"], slots)


@pytest.mark.parametrize("slots", [False, True])
@pytest.mark.parametrize("curve", B.CURVES)
def test_fixture_on_every_curve(ctx, fx, curve, slots):
    cv = ctx.curve(curve)
    check_fixture(cv, fx[curve], curve, slots)
    check_fixture(cv, {"verify": fx[curve]["verify"][:6], "sign": fx[curve]["sign"]}, curve, slots, alg=A.SIG_DBIGN)
    cv.free()


def test_fixture_on_a_handle_from_parameters(ctx, fx):
    cv = libecc_amd.Curve(ctx, params=O.CURVES["BIGN256V1"])
    check_fixture(cv, fx["BIGN256V1"], "BIGN256V1", False)
    check_fixture(cv, fx["BIGN256V1"], "BIGN256V1", True)
    cv.free()


@pytest.mark.parametrize("n", [1, 63, 65, 200])
def test_chunks_and_bad_items_at_the_boundaries(ctx, fx, n):
    curve = "BIGN256V1"
    cv = ctx.curve(curve)
    ql = O.qlen(curve)
    ver = [i for i in fx[curve]["verify"] if i["hash"] == "BELT" and i["oid"] == B.OID_BELT.hex()]
    good = [i for i in ver if i["ret"] == 0]
    bad = [i for i in ver if i["ret"] != 0]
    assert good and bad
    where = {0, 63, 64, 127, 128, n - 1}
    items = [(bad[j % len(bad)] if j in where else good[j % len(good)]) for j in range(n)]
    ctx.set_max_chunk(64)
    try:
        for slots in (False, True):
            got = run_verify(cv, items, slots)
            assert got == [0 if i["ret"] == 0 else 1 for i in items], (n, slots)
        sg = [i for i in fx[curve]["sign"] if i["hash"] == "BELT"]
        sgood, sbad = [i for i in sg if i["ret"] == 0], [i for i in sg if i["ret"] != 0]
        items = [(sbad[j % len(sbad)] if j in where else sgood[j % len(sgood)]) for j in range(n)]
        for (st, sig), i in zip(run_sign(cv, items, True, ql), items):
            assert (st, sig) == ((0, bytes.fromhex(i["out"])) if i["ret"] == 0 else (1, bytes(ql // 2 + ql)))
        # a message slot whose length does not fit the stride rejects its own item and nothing else
        msgs = [bytes.fromhex(i["msg"]) for i in good]
        stride = B.stride_for(max(len(m) for m in msgs))
        sl = [B.slot(m, stride) for m in msgs]
        sl[0] = B.slot(msgs[0], stride, length=stride - 3)
        res = cv.bign_verify(A.SIG_BIGN, 16, b"".join(bytes.fromhex(i["pub"]) for i in good), b"".join(bytes.fromhex(i["sig"]) for i in good),
                             b"".join(sl), stride, B.OID_BELT)
        assert res == bytes([1] + [0] * (len(good) - 1))
        # ... and so in signing: status 1 and an all-zero signature for that item, the recorded bytes for the others
        sgood = [i for i in sgood if i["oid"] == B.OID_BELT.hex()]
        assert len(sgood) > 1
        msgs = [bytes.fromhex(i["msg"]) for i in sgood]
        stride = B.stride_for(max(len(m) for m in msgs))
        sl = [B.slot(m, stride) for m in msgs]
        at = len(sgood) - 1
        sl[at] = B.slot(msgs[at], stride, length=stride - 3)
        sigs, st = cv.bign_sign(A.SIG_BIGN, 16, b"".join(bytes.fromhex(i["x"])[-ql:] for i in sgood),
                                b"".join(bytes.fromhex(i["k"])[-ql:] for i in sgood), b"".join(sl), stride, B.OID_BELT)
        assert st == bytes([0] * at + [1])
        assert sigs == b"".join(bytes.fromhex(i["out"]) for i in sgood[:at]) + bytes(ql // 2 + ql)
    finally:
        ctx.set_max_chunk(1 << 20)
        cv.free()


@pytest.mark.parametrize("curve", B.CURVES)
def test_sign_then_verify_on_the_device(ctx, curve):
    import torch
    cv = ctx.curve(curve)
    ql, cl = O.qlen(curve), O.clen(curve)
    n = 256
    rng = np.random.default_rng(7)
    pubs, xs, ks, msgs = B.random_batch(curve, n, rng)
    privs, nonces = b"".join(be(x, ql) for x in xs), b"".join(be(k, ql) for k in ks)
    stride = B.stride_for(24)
    slots = b"".join(B.slot(m, stride) for m in msgs)
    ctx.set_secret_scalars(False)
    sig0, st0 = cv.bign_sign(A.SIG_BIGN, 16, privs, nonces, slots, stride, B.OID_BELT)
    ctx.set_secret_scalars(True)
    try:
        sig1, st1 = cv.bign_sign(A.SIG_DBIGN, 16, privs, nonces, slots, stride, B.OID_BELT)
    finally:
        ctx.set_secret_scalars(False)
    assert st0 == bytes(n) and (sig1, st1) == (sig0, st0)
    # the digest mode gives the same bytes
    dgs = b"".join(B.belt_hash(m) for m in msgs)
    assert cv.bign_sign(A.SIG_BIGN, 0, privs, nonces, dgs, 32, B.OID_BELT) == (sig0, st0)
    allpub = b"".join(pubs)
    assert cv.bign_verify(A.SIG_BIGN, 16, allpub, sig0, slots, stride, B.OID_BELT) == bytes(n)
    assert cv.bign_verify(A.SIG_BIGN, 0, allpub, sig0, dgs, 32, B.OID_BELT) == bytes(n)
    assert cv.bign_verify(A.SIG_BIGN, 16, allpub, sig0, slots, stride, b"") == bytes([1]) * n
    sl = ql // 2 + ql
    for j in (0, 100, n - 1):
        assert (0, sig0[j * sl:(j + 1) * sl]) == B.sign(curve, "BELT", B.OID_BELT, xs[j], ks[j], msgs[j])
    if O.have_ref():
        for j in range(n):
            assert B.ref_sign(curve, "BELT", B.OID_BELT, xs[j], ks[j], msgs[j]) == (0, sig0[j * sl:(j + 1) * sl]), j
            assert B.ref_verify(curve, "BELT", B.OID_BELT, pubs[j], sig0[j * sl:(j + 1) * sl], msgs[j]) == 0
    # the _dev forms on torch buffers
    dev = torch.device("cuda:0")

    def t(bs):
        return torch.frombuffer(bytearray(bs), dtype=torch.uint8).to(dev)

    d_priv, d_non, d_slots, d_pub = t(privs), t(nonces), t(slots), t(allpub)
    d_sig = torch.zeros(n * sl, dtype=torch.uint8, device=dev)
    d_st = torch.ones(n, dtype=torch.uint8, device=dev)
    d_res = torch.ones(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    cv.bign_sign_dev(A.SIG_BIGN, 16, n, d_priv.data_ptr(), d_non.data_ptr(), d_slots.data_ptr(), stride, B.OID_BELT, d_sig.data_ptr(),
                     d_st.data_ptr(), stream)
    cv.bign_verify_dev(A.SIG_BIGN, 16, n, d_pub.data_ptr(), d_sig.data_ptr(), d_slots.data_ptr(), stride, B.OID_BELT, d_res.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bytes(d_sig.cpu().numpy()) == sig0 and bytes(d_st.cpu().numpy()) == st0 and bytes(d_res.cpu().numpy()) == bytes(n)
    assert ctx.L.ecamd_ctx_wipe_scratch(ctx.h) == 0
    cv.free()


def test_u_zero_and_hbar_zero_at_the_entry_point(ctx):
    rng = np.random.default_rng(11)
    for curve in B.CURVES:
        cv = ctx.curve(curve)
        ql = O.qlen(curve)
        hs = max(32, ql)
        pub, sig, dg = B.u_zero_accepted(curve, B.OID_BELT, rng, hsize=hs)
        assert cv.bign_verify(A.SIG_BIGN, 0, pub, sig, dg, hs, B.OID_BELT) == b"\0"
        assert cv.bign_verify(A.SIG_BIGN, 0, pub, sig[:1] + bytes([sig[1] ^ 1]) + sig[2:], dg, hs, B.OID_BELT) == b"\1"
        q = O.CURVES[curve]["q"]
        x, k = 1 + B.rand_int(rng, q - 1), 1 + B.rand_int(rng, q - 1)
        dz = B.hbar_zero_digest(curve, hs)
        assert int.from_bytes(dz, "little") % q == 0
        sigs, st = cv.bign_sign(A.SIG_BIGN, 0, be(x, ql), be(k, ql), dz, hs, B.OID_BELT)
        assert (st[0], sigs) == B.sign_digest(curve, B.OID_BELT, x, k, dz)
        cv.free()


def test_existing_calls_are_untouched_and_argument_errors(ctx, fx):
    import os
    curve = "SECP256R1"
    cv = ctx.curve(curve)
    hfx = S.load_fixture(os.path.join(O.GOLDEN, "sig_hashed.json"))[curve]["ECKCDSA"]["verify"]
    items = [i for i in hfx if i["hash"] == "SHA256"]

    def kcdsa():
        return cv.sig_hashed_verify(S.ECKCDSA, 2, b"".join(bytes.fromhex(i["pub"]) for i in items), b"".join(bytes.fromhex(i["sig"]) for i in items),
                                    b"".join(S.kcdsa_h(curve, "SHA256", bytes.fromhex(i["pub"]), bytes.fromhex(i["msg"])) for i in items), 32)

    before = kcdsa()
    assert before == bytes(0 if i["ret"] == 0 else 1 for i in items) and 0 in before and 1 in before
    check_fixture(cv, {"verify": fx[curve]["verify"][:8], "sign": fx[curve]["sign"][:4]}, curve, True)
    assert kcdsa() == before
    assert ctx.L.ecamd_ctx_wipe_scratch(ctx.h) == 0
    i = fx[curve]["verify"][0]
    pub, sig, dg = bytes.fromhex(i["pub"]), bytes.fromhex(i["sig"]), B.H(i["hash"], bytes.fromhex(i["msg"]))
    L = cv.L
    res = C.create_string_buffer(1)
    for alg, ht, stride, oid, ol in ((17, 0, len(dg), B.OID_BELT, 11), (2, 0, len(dg), B.OID_BELT, 11), (18, 5, 36, B.OID_BELT, 11),
                                     (18, 17, 36, B.OID_BELT, 11), (18, 0, len(dg), bytes(65), 65), (18, 0, len(dg), None, 3),
                                     (18, 0, 0, B.OID_BELT, 11), (18, 0, 129, B.OID_BELT, 11), (18, 16, 34, B.OID_BELT, 11)):
        assert L.ec_bign_verify_batch(ctx.h, cv.h, alg, ht, 1, pub, sig, dg, stride, oid, ol, res) == -1, (alg, ht, stride, ol)
        assert L.ecamd_last_error().decode().startswith("ec_bign_verify_batch:")
        st = C.create_string_buffer(1)
        so = C.create_string_buffer(len(sig))
        assert L.ec_bign_sign_batch(ctx.h, cv.h, alg, ht, 1, bytes(32), bytes(31) + b"\1", dg, stride, oid, ol, so, st) == -1
    other = libecc_amd.Context(0)
    try:
        assert L.ec_bign_verify_batch(other.h, cv.h, 18, 0, 1, pub, sig, dg, len(dg), B.OID_BELT, 11, res) == -1
    finally:
        other.close()
    assert L.ec_bign_verify_batch(ctx.h, cv.h, 18, 0, 0, None, None, None, 32, B.OID_BELT, 11, None) == 0
    assert cv.bign_verify(A.SIG_BIGN, 0, pub, sig, dg, len(dg), B.OID_BELT) == b"\0"
    cv.free()
