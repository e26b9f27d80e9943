"""GPU tests of deterministic ECDSA (ec_rfc6979_nonce_batch, ec_decdsa_sign_batch and their _dev forms): the 32 RFC 6979 vectors of
the reference, the recorded answers of the unmodified reference (tests/golden/decdsa.json) and the Python restatement with a retry
counter (tests/decdsa_ref.py)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import libecc_amd
import oracles as O
import decdsa_ref as D
import sigfam_ref as R
from bign_ref import fast_mul

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = libecc_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return D.load_fixture(os.path.join(O.GOLDEN, "decdsa.json"))


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(O.GOLDEN, "ecdsa_kats.json")) as f:
        return [v for v in json.load(f) if v["sig_type"] == "DECDSA"]


def expected(curve, i):
    """(status, signature bytes) of a fixture item: the reference's bytes, or status 1 and zeros where it fails"""
    return (0, bytes.fromhex(i["sig"])) if i["ret"] == 0 else (1, bytes(2 * O.qlen(curve)))


def sign_items(cv, h, privs, msgs, slots):
    """one ec_decdsa_sign_batch call: [(status, signature)]"""
    ql = cv.qlen
    if slots:
        stride = D.stride_for(max(len(m) for m in msgs))
        inp = b"".join(D.slot(m, stride) for m in msgs)
    else:
        stride, inp = D.HSIZE[h], b"".join(D.H(h, m) for m in msgs)
    sigs, st = cv.decdsa_sign(D.HT[h], b"".join(privs), inp, stride, not slots)
    return [(st[j], sigs[2 * ql * j:2 * ql * (j + 1)]) for j in range(len(privs))]


@functools.lru_cache(maxsize=None)
def pub_of(curve, x):
    c = O.CURVES[curve]
    return R.pt_bytes(curve, fast_mul(x, (c["gx"], c["gy"]), c["a"], c["p"]))


def assert_all_verify(cv, curve, h, privs, msgs, got):
    """every signature the device produced (status 0) is accepted by ec_ecdsa_verify_batch; x = 0 signs in the reference but has no
    public key to verify under"""
    sel = [j for j, (st, _) in enumerate(got) if st == 0 and int.from_bytes(privs[j], "big") != 0]
    assert sel
    res = cv.ecdsa_verify(b"".join(pub_of(curve, int.from_bytes(privs[j], "big")) for j in sel), b"".join(got[j][1] for j in sel),
                          b"".join(D.H(h, msgs[j]) for j in sel), D.HSIZE[h])
    assert res == bytes(len(sel)), (curve, h)


def interleaved(items):
    """the fixture's items of one hash reordered so that every failing key sits between two good ones"""
    good, bad = [i for i in items if i["ret"] == 0], [i for i in items if i["ret"] != 0]
    assert bad and len(good) > len(bad)
    out = []
    for j, b in enumerate(bad):
        out += [good[j], b]
    out += good[len(bad):]
    for j, i in enumerate(out):
        if i["ret"] != 0:
            assert 0 < j < len(out) - 1 and out[j - 1]["ret"] == 0 and out[j + 1]["ret"] == 0
    return out


@pytest.mark.parametrize("slots", [True, False])
def test_rfc6979_vectors(ctx, kats, slots):
    assert len(kats) == 32
    for curve in sorted({v["curve"] for v in kats}):
        cv = ctx.curve(curve)
        for h in sorted({v["hash"] for v in kats if v["curve"] == curve}):
            sel = [v for v in kats if v["curve"] == curve and v["hash"] == h]
            privs = [bytes.fromhex(v["priv_key"]).rjust(cv.qlen, b"\0")[-cv.qlen:] for v in sel]
            msgs = [bytes.fromhex(v["msg"]) for v in sel]
            got = sign_items(cv, h, privs, msgs, slots)
            assert got == [(0, bytes.fromhex(v["exp_sig"])) for v in sel], (curve, h, slots)
            assert_all_verify(cv, curve, h, privs, msgs, got)
        cv.free()


@pytest.mark.parametrize("curve", D.CURVES)
def test_fixture_host_pointers(ctx, fx, curve):
    """signatures and status byte-exact; every failing key (x >= q) sits between two good ones, whose bytes are the recorded ones"""
    cv = ctx.curve(curve)
    ql = cv.qlen
    for h in D.HASHES:
        items = interleaved([i for i in fx[curve] if i["hash"] == h])
        privs, msgs = [bytes.fromhex(i["x"]) for i in items], [bytes.fromhex(i["msg"]) for i in items]
        for slots in (True, False):
            got = sign_items(cv, h, privs, msgs, slots)
            assert got == [expected(curve, i) for i in items], (curve, h, slots)
            assert_all_verify(cv, curve, h, privs, msgs, got)
        # the nonces themselves: the restatement's and oracles.rfc6979_nonce's
        ks, st = cv.rfc6979_nonce(D.HT[h], b"".join(privs), b"".join(D.H(h, m) for m in msgs))
        assert st == bytes(len(items))
        assert ks == b"".join(bytes.fromhex(i["k"]) for i in items), (curve, h)
        assert ks == b"".join(O.rfc6979_nonce(curve, h, p, m).to_bytes(ql, "big") for p, m in zip(privs, msgs))
    cv.free()


@pytest.mark.parametrize("curve", D.CURVES)
def test_fixture_device_pointers(ctx, fx, curve):
    import torch
    dev = torch.device("cuda:0")

    def t(bs):
        return torch.frombuffer(bytearray(bs), dtype=torch.uint8).to(dev)

    cv = ctx.curve(curve)
    ql = cv.qlen
    stream = torch.cuda.current_stream().cuda_stream
    for h in D.HASHES:
        items = interleaved([i for i in fx[curve] if i["hash"] == h])
        n = len(items)
        privs, msgs = [bytes.fromhex(i["x"]) for i in items], [bytes.fromhex(i["msg"]) for i in items]
        stride = D.stride_for(max(len(m) for m in msgs))
        d_priv, d_dig = t(b"".join(privs)), t(b"".join(D.H(h, m) for m in msgs))
        d_slots = t(b"".join(D.slot(m, stride) for m in msgs))
        want = [expected(curve, i) for i in items]
        for d_in, st_, dig in ((d_slots, stride, False), (d_dig, D.HSIZE[h], True)):
            d_sig = torch.full((n * 2 * ql,), 0xEE, dtype=torch.uint8, device=dev)
            d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
            cv.decdsa_sign_dev(D.HT[h], n, d_priv.data_ptr(), d_in.data_ptr(), st_, dig, d_sig.data_ptr(), d_st.data_ptr(), stream)
            torch.cuda.synchronize()
            sig, st = bytes(d_sig.cpu().numpy()), bytes(d_st.cpu().numpy())
            got = [(st[j], sig[2 * ql * j:2 * ql * (j + 1)]) for j in range(n)]
            assert got == want, (curve, h, dig)
            assert_all_verify(cv, curve, h, privs, msgs, got)
        d_k = torch.full((n * ql,), 0xEE, dtype=torch.uint8, device=dev)
        d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        cv.rfc6979_nonce_dev(D.HT[h], n, d_priv.data_ptr(), d_dig.data_ptr(), d_k.data_ptr(), d_st.data_ptr(), stream)
        torch.cuda.synchronize()
        assert bytes(d_k.cpu().numpy()) == b"".join(bytes.fromhex(i["k"]) for i in items) and bytes(d_st.cpu().numpy()) == bytes(n)
    assert ctx.L.ecamd_ctx_wipe_scratch(ctx.h) == 0
    cv.free()


@pytest.fixture(scope="module")
def mixed_waves():
    """BRAINPOOLP384R1 / SHA-256, n = 197 (three full waves and a partial one): items chosen so that every wave holds retry counts
    0, 1 and >= 2 side by side; computed once"""
    curve, h, n = "BRAINPOOLP384R1", "SHA256", 197
    q, ql = O.CURVES[curve]["q"], O.qlen(curve)
    rng = np.random.default_rng(197)
    privs, msgs, ks, rs = [], [], [], []
    while len(privs) < n:
        want = len(privs) % 3                      # 0, 1, >= 2 in turn
        x, m = (1 + R.rand_int(rng, q - 1)).to_bytes(ql, "big"), rng.integers(0, 256, size=int(rng.integers(0, 60)), dtype=np.uint8).tobytes()
        k, r = D.nonce(curve, h, x, m)
        if min(r, 2) == want:
            privs.append(x); msgs.append(m); ks.append(k); rs.append(r)
    for w in range(0, n, 64):
        assert {min(r, 2) for r in rs[w:w + 64]} == {0, 1, 2}
    sigs = [D.sign_with(curve, int.from_bytes(x, "big"), k, D.H(h, m)) for x, k, m in zip(privs, ks, msgs)]
    return curve, h, privs, msgs, ks, sigs


def test_retries_mixed_inside_every_wave(ctx, mixed_waves):
    curve, h, privs, msgs, ks, sigs = mixed_waves
    cv = ctx.curve(curve)
    ql = cv.qlen
    dgs = b"".join(D.H(h, m) for m in msgs)
    try:
        for chunk in (1 << 20, 64):
            ctx.set_max_chunk(chunk)
            got, st = cv.rfc6979_nonce(D.HT[h], b"".join(privs), dgs)
            assert st == bytes(len(privs)) and got == b"".join(k.to_bytes(ql, "big") for k in ks), chunk
            for slots in (True, False):
                got = sign_items(cv, h, privs, msgs, slots)
                assert got == sigs, (chunk, slots)
    finally:
        ctx.set_max_chunk(1 << 20)
    assert_all_verify(cv, curve, h, privs, msgs, got)
    cv.free()


def test_secret_scalar_mode_gives_the_same_bytes(ctx, fx, mixed_waves):
    curve, h, privs, msgs, ks, sigs = mixed_waves
    ctx.set_secret_scalars(True)
    try:
        cv = ctx.curve(curve)
        got = sign_items(cv, h, privs, msgs, True)
        assert got == sigs
        assert_all_verify(cv, curve, h, privs, msgs, got)
        cv.free()
        for c2 in ("SECP256R1", "SECP521R1", "SECP224K1"):
            cv = ctx.curve(c2)
            items = [i for i in fx[c2] if i["hash"] == "SHA512"]
            privs2, msgs2 = [bytes.fromhex(i["x"]) for i in items], [bytes.fromhex(i["msg"]) for i in items]
            got = sign_items(cv, "SHA512", privs2, msgs2, False)
            assert got == [expected(c2, i) for i in items], c2
            assert_all_verify(cv, c2, "SHA512", privs2, msgs2, got)
            cv.free()
    finally:
        ctx.set_secret_scalars(False)


def test_bad_slot_rejects_its_own_item_only(ctx, fx):
    curve, h = "SECP256R1", "SHA256"
    cv = ctx.curve(curve)
    items = [i for i in fx[curve] if i["hash"] == h and i["ret"] == 0]
    msgs = [bytes.fromhex(i["msg"]) for i in items]
    stride = D.stride_for(max(len(m) for m in msgs))
    sl = [D.slot(m, stride) for m in msgs]
    for j, ln in ((0, stride - 3), (3, 0xFFFFFFFF), (len(items) - 1, stride)):
        sl[j] = D.slot(msgs[j], stride, length=ln)
    sigs, st = cv.decdsa_sign(D.HT[h], b"".join(bytes.fromhex(i["x"]) for i in items), b"".join(sl), stride, False)
    for j, i in enumerate(items):
        want = (1, bytes(64)) if j in (0, 3, len(items) - 1) else (0, bytes.fromhex(i["sig"]))
        assert (st[j], sigs[64 * j:64 * j + 64]) == want, j
    cv.free()


def test_call_level_arguments(ctx):
    cv = ctx.curve("SECP256R1")
    L = ctx.L
    priv, dg = bytes([1] * 32), bytes(64)
    k, st, sig = C.create_string_buffer(32), C.create_string_buffer(b"\x07", 1), C.create_string_buffer(64)
    # n = 0: nothing touched, NULL pointers welcome
    assert L.ec_rfc6979_nonce_batch(ctx.h, cv.h, 2, 0, None, None, None, None) == 0
    assert L.ec_decdsa_sign_batch(ctx.h, cv.h, 2, 0, None, None, 32, 1, None, None) == 0
    assert L.ec_rfc6979_nonce_batch_dev(ctx.h, cv.h, 2, 0, None, None, None, None, None) == 0
    assert L.ec_decdsa_sign_batch_dev(ctx.h, cv.h, 2, 0, None, None, 8, 0, None, None, None) == 0
    assert st.raw == b"\x07"
    for ht in (0, 5, 16, -1):
        assert L.ec_rfc6979_nonce_batch(ctx.h, cv.h, ht, 1, priv, dg, k, st) == -1
        assert b"hash_type" in L.ecamd_last_error()
        assert L.ec_decdsa_sign_batch(ctx.h, cv.h, ht, 1, priv, dg, 32, 1, sig, st) == -1
        assert L.ec_rfc6979_nonce_batch_dev(ctx.h, cv.h, ht, 0, None, None, None, None, None) == -1
        assert L.ec_decdsa_sign_batch_dev(ctx.h, cv.h, ht, 0, None, None, 32, 1, None, None, None) == -1
    # NULL arguments with n > 0, NULL handles
    assert L.ec_rfc6979_nonce_batch(ctx.h, cv.h, 2, 1, None, dg, k, st) == -1
    assert L.ec_rfc6979_nonce_batch(ctx.h, cv.h, 2, 1, priv, dg, None, st) == -1
    assert L.ec_decdsa_sign_batch(ctx.h, cv.h, 2, 1, priv, None, 32, 1, sig, st) == -1
    assert L.ec_decdsa_sign_batch(ctx.h, cv.h, 2, 1, priv, dg, 32, 1, sig, None) == -1
    assert L.ec_decdsa_sign_batch(None, cv.h, 2, 1, priv, dg, 32, 1, sig, st) == -1
    assert L.ec_decdsa_sign_batch(ctx.h, None, 2, 1, priv, dg, 32, 1, sig, st) == -1
    assert L.ec_decdsa_sign_batch_dev(ctx.h, cv.h, 2, 1, None, None, 32, 1, None, None, None) == -1
    # strides: digest mode wants hsize exactly; slot mode a multiple of 4 in 4 .. 4096; in_is_digest 0 or 1
    for stride, dig in ((28, 1), (64, 1), (0, 1), (6, 0), (0, 0), (4100, 0), (32, 2)):
        assert L.ec_decdsa_sign_batch(ctx.h, cv.h, 2, 1, priv, dg, stride, dig, sig, st) == -1, (stride, dig)
        assert len(L.ecamd_last_error()) > 0
    assert st.raw == b"\x07" and sig.raw == bytes(64)
    assert L.ec_decdsa_sign_batch(ctx.h, cv.h, 2, 1, priv, dg, 32, 1, sig, st) == 0 and st.raw == b"\x00"
    cv.free()
