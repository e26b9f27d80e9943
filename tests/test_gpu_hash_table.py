"""GPU tests of ec_digest_slots_batch / ec_digest_slots_batch_dev / ecamd_digest_len: SHA3-224 / 256 / 384 / 512, SHA-512/224,
SHA-512/256, RIPEMD-160 and BASH224 / 256 / 384 / 512 on the device against the recorded reference answers of
tests/golden/hash_table.json; mixed block counts in one wave, chunks, the _dev form, slots that do not fit, the numbers the older call
serves, the protocols fed with on-device digests (BIGN and DBIGN with BASH, ECDSA with SHA-3), and the call-level errors.  All
comparisons are exact bytes."""
import ctypes as C
import json
import os

import pytest

import oracles as O
import hashtable_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return T.load_fixture()


@pytest.fixture(scope="module")
def kats(fx):
    return T.kat_table(fx)


@pytest.fixture(scope="module")
def ctx():
    import libecc_amd
    c = libecc_amd.Context(0)
    yield c
    c.close()


def to_dev(bs):
    import torch
    return torch.frombuffer(bytearray(bs), dtype=torch.uint8).to(torch.device("cuda:0"))


def from_dev(t):
    return bytes(t.cpu().numpy())


@pytest.mark.parametrize("name", list(T.TABLE))
def test_kats(ctx, kats, name):
    lens = T.kat_lengths(name)
    got = ctx.digest_slots(T.HASH_IDS[name], T.pack_slots([T.counting(n) for n in lens], 4096), 4096)
    hl = T.HASH_SIZES[name]
    for j, n in enumerate(lens):
        assert got[j * hl:(j + 1) * hl] == kats[name][n], (name, n)
    assert len(got) == hl * len(lens)
    # each alone, in the smallest slot that holds it
    for n in lens:
        assert ctx.digest_slots(T.HASH_IDS[name], T.slot(T.counting(n), (4 + n + 3) & ~3), (4 + n + 3) & ~3) == kats[name][n], (name, n)


@pytest.mark.parametrize("name", list(T.TABLE))
def test_mixed_lengths_chunks_and_wave_edges(ctx, kats, name):
    ks = T.kat_lengths(name)
    lens = [ks[i % len(ks)] for i in range(130)]
    slots = T.pack_slots([T.counting(n) for n in lens], 4096)
    exp = b"".join(kats[name][n] for n in lens)
    if T.have_hashlib(name):
        assert exp == b"".join(T.py_hash(name, T.counting(n)) for n in lens)
    ctx.set_max_chunk(64)       # three chunks, the last one ragged
    try:
        assert ctx.digest_slots(T.HASH_IDS[name], slots, 4096) == exp
    finally:
        ctx.set_max_chunk(1 << 20)
    assert ctx.digest_slots(T.HASH_IDS[name], slots, 4096) == exp


def test_dev_form_and_overlong_slot(ctx, kats):
    import torch
    dev = torch.device("cuda:0")
    for name in T.TABLE:
        lens = [n for n in T.kat_lengths(name) if n <= 300]
        slots = bytearray(T.pack_slots([T.counting(n) for n in lens], 304))
        bad = len(lens) // 2
        slots[bad * 304:bad * 304 + 4] = (301).to_bytes(4, "little")       # 4 + 301 > 304
        hl, n = T.HASH_SIZES[name], len(lens)
        d_in = to_dev(slots)
        d_out = torch.full((n * hl + 8,), 0xAA, dtype=torch.uint8, device=dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        ctx.digest_slots_dev(T.HASH_IDS[name], n, d_in.data_ptr(), 304, d_out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        exp = b"".join(bytes(hl) if j == bad else kats[name][m] for j, m in enumerate(lens))
        assert from_dev(d_out) == exp + b"\xaa" * 8, name
        assert from_dev(d_in) == bytes(slots)


def test_old_numbers_agree_with_hash_slots(ctx):
    lens = [0, 1, 31, 32, 55, 56, 63, 64, 65, 111, 112, 127, 128, 129, 200, 256] * 5
    msgs = [T.counting(n)[::-1] for n in lens]
    slots = T.pack_slots(msgs, 264)
    for ht, hl in T.OLD_IDS.items():
        got = ctx.digest_slots(ht, slots, 264)
        assert len(got) == hl * len(lens) and got == ctx.hash_slots(ht, slots, 264), ht
        # ... and here a slot that does not fit gives zeros for these numbers too
        bad = bytearray(slots)
        bad[3 * 264:3 * 264 + 4] = (261).to_bytes(4, "little")
        got2 = ctx.digest_slots(ht, bytes(bad), 264)
        assert got2 == got[:3 * hl] + bytes(hl) + got[4 * hl:], ht


def digests_on_device(ctx, name, msgs, stream):
    """ec_digest_slots_batch_dev into a fresh device buffer, enqueued on `stream`: (the buffer, the digest length)"""
    import torch
    stride = T.stride_for(msgs)
    d_slots = to_dev(T.pack_slots(msgs, stride))
    hl = T.HASH_SIZES[name]
    d_dg = torch.zeros(len(msgs) * hl, dtype=torch.uint8, device=d_slots.device)
    torch.cuda.synchronize()        # the fills above run on torch's stream, the library on the one it is handed
    ctx.digest_slots_dev(T.HASH_IDS[name], len(msgs), d_slots.data_ptr(), stride, d_dg.data_ptr(), stream)
    return d_dg, hl


@pytest.mark.parametrize("curve,name", [("BIGN384V1", "BASH384"), ("BIGN512V1", "BASH512")])
def test_bign_with_bash_digests_from_the_device(ctx, fx, curve, name):
    import torch
    import libecc_amd.api as A
    dev = torch.device("cuda:0")
    items = fx["items"]["BIGN/%s/%s" % (curve, name)]
    ditems = fx["items"].get("DBIGN/%s/%s" % (curve, name), [])
    oid = T.OID_BASH[name]
    cv = ctx.curve(curve)
    try:
        n, sl = len(items), cv.bign_siglen()
        tstream = torch.cuda.Stream(device=dev)
        stream = tstream.cuda_stream
        d_pub = to_dev(b"".join(bytes.fromhex(i["pub"]) for i in items))
        d_sig = to_dev(b"".join(bytes.fromhex(i["sig"]) for i in items))
        d_res = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        d_x = to_dev(b"".join(bytes.fromhex(i["x"]) for i in items))
        d_k = to_dev(b"".join(bytes.fromhex(i["k"]) for i in items))
        d_out = torch.zeros(n * sl, dtype=torch.uint8, device=dev)
        d_st = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        d_dg, hl = digests_on_device(ctx, name, [bytes.fromhex(i["msg"]) for i in items], stream)
        cv.bign_verify_dev(A.SIG_BIGN, 0, n, d_pub.data_ptr(), d_sig.data_ptr(), d_dg.data_ptr(), hl, oid, d_res.data_ptr(), stream)
        cv.bign_sign_dev(A.SIG_BIGN, 0, n, d_x.data_ptr(), d_k.data_ptr(), d_dg.data_ptr(), hl, oid, d_out.data_ptr(), d_st.data_ptr(), stream)
        torch.cuda.synchronize()
        assert from_dev(d_res) == bytes(0 if i["ret"] == 0 else 1 for i in items)
        assert from_dev(d_st) == bytes(n)
        assert from_dev(d_out) == b"".join(bytes.fromhex(i["signed"]) for i in items)
        assert from_dev(d_dg) == b"".join(T.shim_hash(name, bytes.fromhex(i["msg"])) for i in items)
        if ditems:
            # DBIGN: the nonce is derived on the device from the same on-device digests; the bytes are the reference's deterministic ones
            n = len(ditems)
            d_x = to_dev(b"".join(bytes.fromhex(i["x"]) for i in ditems))
            d_out = torch.zeros(n * sl, dtype=torch.uint8, device=dev)
            d_st = torch.full((n,), 7, dtype=torch.uint8, device=dev)
            d_pub = to_dev(b"".join(bytes.fromhex(i["pub"]) for i in ditems))
            d_sig = to_dev(b"".join(bytes.fromhex(i["sig"]) for i in ditems))
            d_res = torch.full((n,), 7, dtype=torch.uint8, device=dev)
            d_dg, hl = digests_on_device(ctx, name, [bytes.fromhex(i["msg"]) for i in ditems], stream)
            cv.dbign_sign_dev(0, n, d_x.data_ptr(), d_dg.data_ptr(), hl, oid, b"", d_out.data_ptr(), d_st.data_ptr(), stream)
            cv.bign_verify_dev(A.SIG_DBIGN, 0, n, d_pub.data_ptr(), d_sig.data_ptr(), d_dg.data_ptr(), hl, oid, d_res.data_ptr(), stream)
            torch.cuda.synchronize()
            assert from_dev(d_st) == bytes(n)
            assert from_dev(d_out) == b"".join(bytes.fromhex(i["signed"]) for i in ditems)
            assert from_dev(d_res) == bytes(0 if i["ret"] == 0 else 1 for i in ditems)
    finally:
        cv.free()


def ecdsa_on_device(ctx, curve, name, items):
    """(verdicts, signatures, status) of ec_ecdsa_verify_batch_dev / ec_ecdsa_sign_batch_dev behind ec_digest_slots_batch_dev; items:
    [(pub, sig, x, k, msg)]"""
    import torch
    dev = torch.device("cuda:0")
    cv = ctx.curve(curve)
    try:
        n = len(items)
        tstream = torch.cuda.Stream(device=dev)
        stream = tstream.cuda_stream
        d_pub, d_sig = to_dev(b"".join(i[0] for i in items)), to_dev(b"".join(i[1] for i in items))
        d_x, d_k = to_dev(b"".join(i[2] for i in items)), to_dev(b"".join(i[3] for i in items))
        d_res = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        d_out = torch.zeros(n * 2 * cv.qlen, dtype=torch.uint8, device=dev)
        d_st = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        d_dg, hl = digests_on_device(ctx, name, [i[4] for i in items], stream)
        cv.ecdsa_verify_dev(n, d_pub.data_ptr(), d_sig.data_ptr(), d_dg.data_ptr(), hl, d_res.data_ptr(), stream)
        cv.ecdsa_sign_dev(n, d_x.data_ptr(), d_k.data_ptr(), d_dg.data_ptr(), hl, d_out.data_ptr(), d_st.data_ptr(), stream)
        torch.cuda.synchronize()
        assert from_dev(d_dg) == b"".join(T.py_hash(name, i[4]) for i in items), (curve, name)
        return from_dev(d_res), from_dev(d_out), from_dev(d_st)
    finally:
        cv.free()


@pytest.mark.parametrize("curve,name", [("SECP256R1", "SHA3_256"), ("SECP384R1", "SHA3_384")])
def test_ecdsa_with_sha3_digests_from_the_device(ctx, fx, curve, name):
    items = fx["items"]["ECDSA/%s/%s" % (curve, name)]
    hx = bytes.fromhex
    res, sigs, st = ecdsa_on_device(ctx, curve, name, [(hx(i["pub"]), hx(i["sig"]), hx(i["x"]), hx(i["k"]), hx(i["msg"])) for i in items])
    assert res == bytes(0 if i["ret"] == 0 else 1 for i in items)
    assert st == bytes(len(items))
    assert sigs == b"".join(hx(i["signed"]) for i in items)


def test_the_references_own_ecdsa_sha3_vectors(ctx):
    """the ECDSA known answers of the reference's self tests that use SHA-3 (tests/golden/ecdsa_kats.json holds five): the recorded
    signature verifies under the key derived on the device, and signing with the recorded nonce gives its bytes"""
    with open(os.path.join(O.GOLDEN, "ecdsa_kats.json")) as f:
        kats = [k for k in json.load(f) if k["sig_type"] == "ECDSA" and k["hash"] in T.TABLE and k["k"]]
    assert len(kats) == 5 and {k["hash"] for k in kats} == {"SHA3_224", "SHA3_256", "SHA3_384", "SHA3_512"}
    for k in kats:
        cv = ctx.curve(k["curve"])
        try:
            ql = cv.qlen
            x = bytes.fromhex(k["priv_key"]).rjust(ql, b"\0")[-ql:]
            pub, st = cv.scalar_mult(x)
            assert st == b"\0"
        finally:
            cv.free()
        nonce = int(k["k"], 16).to_bytes(ql, "big")
        sig = bytes.fromhex(k["exp_sig"])
        res, out, st = ecdsa_on_device(ctx, k["curve"], k["hash"], [(pub, sig, x, nonce, bytes.fromhex(k["msg"]))])
        assert (res, out, st) == (b"\0", sig, b"\0"), k["name"]


def test_call_level_errors_and_lengths(ctx):
    L = ctx.L
    slots = T.slot(b"abc", 40)
    for ht in (0, 12, 16, 21, -1):
        assert L.ecamd_digest_len(ht) == 0
        out = C.create_string_buffer(b"\x55" * 64, 64)
        assert L.ec_digest_slots_batch(ctx.h, ht, 1, slots, 40, out) == -1 and "hash_type" in L.ecamd_last_error().decode(), ht
        assert L.ec_digest_slots_batch_dev(ctx.h, ht, 1, None, 40, None, None) == -1 and "hash_type" in L.ecamd_last_error().decode(), ht
        assert out.raw == b"\x55" * 64
    for ht, hl in T.ALL_SIZES.items():
        assert L.ecamd_digest_len(ht) == hl, ht
    assert sorted(T.ALL_SIZES) == [h for h in range(-2, 40) if L.ecamd_digest_len(h)]
    for stride in (0, 2, 6, 4100):
        out = C.create_string_buffer(b"\x55" * 64, 64)
        assert L.ec_digest_slots_batch(ctx.h, 6, 1, bytes(4104), stride, out) == -1 and "stride" in L.ecamd_last_error().decode(), stride
        assert L.ec_digest_slots_batch_dev(ctx.h, 19, 1, None, stride, None, None) == -1 and "stride" in L.ecamd_last_error().decode(), stride
        assert out.raw == b"\x55" * 64
    out = C.create_string_buffer(b"\x55" * 64, 64)
    assert L.ec_digest_slots_batch(ctx.h, 6, 1, None, 40, out) == -1
    assert L.ec_digest_slots_batch(ctx.h, 6, 1, slots, 40, None) == -1
    assert L.ec_digest_slots_batch(None, 6, 1, slots, 40, out) == -1
    assert L.ec_digest_slots_batch_dev(ctx.h, 6, 1, None, 40, None, None) == -1
    # n = 0 returns 0 and touches nothing, whatever the pointers
    assert L.ec_digest_slots_batch(ctx.h, 6, 0, None, 40, out) == 0
    assert L.ec_digest_slots_batch(ctx.h, 20, 0, None, 40, None) == 0
    assert L.ec_digest_slots_batch_dev(ctx.h, 15, 0, None, 40, None, None) == 0
    assert out.raw == b"\x55" * 64
    assert ctx.digest_slots(17, b"", 40) == b""
