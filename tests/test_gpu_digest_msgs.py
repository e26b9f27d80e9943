"""ec_digest_msgs_batch, ec_ecdsa_verify_msgs_batch and ec_decdsa_sign_msgs_batch on the device against tests/golden/digest_msgs.json, the
unmodified reference's answers.  A batch has 130 items (two full waves and a tail of two); the fixture's cases are walked round and
round, so the 70 001-octet messages sit among short ones and the lanes of a wave diverge.
  digests     every hash, through the host form in one piece, at max_chunk 64 and with a byte cap that splits the array mid-way, with
              the input cut into call prefix / item prefix / message at digest_msgs_ref.GPU_SPLITS; the _dev form on torch buffers; n = 0
              and empty messages; unusable items; agreement with ec_digest_slots_batch where a slot can hold the message
  protocols   the recorded signatures (both scalar modes) and verdicts; Streebog refused by the signing call in secret-scalar mode
  composition ECKCDSA's published cases of tests/golden/sig_kats.json: item_prefix = z, then ec_sig_hashed_verify_ht_batch_dev
The library's stream is not torch's: device buffers are kept until the test has synchronised."""
import ctypes as C
import os

import pytest

import libecc_amd
import oracles as O
import hashtable_ref as T
import hmac_ht_ref as M
import sigkats_ref as K
import digest_msgs_ref as D

pytestmark = pytest.mark.gpu
N = D.N_GPU
CAP_ENV = "ECAMD_MSGS_CHUNK_BYTES"


@pytest.fixture(scope="module")
def ctx():
    c = libecc_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return D.load_fixture()


def hash_of(name, x):
    """hashlib, or the host build of the unit where hashlib lacks the hash"""
    return M.py_hash(name, x) if M.have_hashlib(name) else D.shim_digest(name, b"", b"", x, 0, len(x))[1]


@pytest.fixture(scope="module")
def want(fx):
    """{hash: the digest of every case}, from the reference where hashlib lacks the hash: the fixture records full digests for the
    message-only variants and tags for all, so the full expectation is the unit's host build, which test_digest_msgs_host.py pins to
    the fixture; here every digest is checked against the fixture's tag and the whole against its sum"""
    out = {}
    for name in D.NAMES:
        digs = []
        for idx in range(len(D.cases(name))):
            x = D.case_stream(name, idx)
            digs.append(hash_of(name, x))
        D.assert_digests(fx, name, digs)
        out[name] = digs
    return out


def to_dev(bs, pad_to=1):
    """the octets on the device, the tensor sized to a multiple of pad_to (at least one element)"""
    import torch
    size = max(pad_to, (len(bs) + pad_to - 1) // pad_to * pad_to)
    return torch.frombuffer(bytearray(bs) + bytearray(size - len(bs)), dtype=torch.uint8).to(torch.device("cuda:0"))


def dev_fill(n, fill):
    import torch
    return torch.full((max(n, 1),), fill, dtype=torch.uint8, device=torch.device("cuda:0"))


def from_dev(t, n):
    return bytes(t.cpu().numpy())[:n]


def sync():
    import torch
    torch.cuda.synchronize()


def offsets_of(lens):
    offs, pos = [0], 0
    for l in lens:
        pos += l
        offs.append(pos)
    return offs


def u64s(vals):
    return b"".join(int(v).to_bytes(8, "little") for v in vals)


def capped(ctx, cap, chunk, fn):
    old = os.environ.get(CAP_ENV)
    try:
        if cap:
            os.environ[CAP_ENV] = str(cap)
        ctx.set_max_chunk(chunk)
        return fn()
    finally:
        ctx.set_max_chunk(1 << 20)
        if cap:
            if old is None:
                del os.environ[CAP_ENV]
            else:
                os.environ[CAP_ENV] = old


@pytest.mark.parametrize("name", D.NAMES)
def test_digests_host_form(ctx, want, name):
    ht, hl = D.HASH_IDS[name], D.HASH_SIZES[name]
    for k, (cpl, ipl) in enumerate(D.GPU_SPLITS):
        idxs, cp, ips, msgs = D.batch(name, cpl, ipl)
        assert any(len(m) > 60000 for m in msgs) and {o & 3 for o in offsets_of(map(len, msgs))[:-1]} == {0, 1, 2, 3}
        exp = b"".join(want[name][i] for i in idxs)
        # one piece; max_chunk 64: three pieces with a ragged last one; a byte cap below one long message: pieces that end mid-array and
        # long messages in pieces of their own.  The message-only split runs all three, the others one each in turn.
        modes = [(0, 1 << 20), (0, 64), (50000, 1 << 20)]
        for cap, chunk in (modes if k == 0 else [modes[k % 3]]):
            dg, st = capped(ctx, cap, chunk, lambda: ctx.digest_msgs(ht, msgs, cp, ips if ipl else None))
            assert st == bytes(N), (name, cpl, ipl, cap, chunk)
            bad = [j for j in range(N) if dg[j * hl:(j + 1) * hl] != exp[j * hl:(j + 1) * hl]]
            assert not bad, (name, cpl, ipl, cap, chunk, [(j, D.cases(name)[idxs[j]]) for j in bad[:6]])


@pytest.mark.parametrize("name", D.NAMES)
def test_digests_dev_form_and_slots(ctx, want, name):
    ht, hl = D.HASH_IDS[name], D.HASH_SIZES[name]
    for cpl, ipl in (D.GPU_SPLITS[0], D.GPU_SPLITS[2]):
        idxs, cp, ips, msgs = D.batch(name, cpl, ipl)
        packed = b"".join(msgs)
        d_msgs, d_offs = to_dev(packed, 4), to_dev(u64s(offsets_of(map(len, msgs))), 8)
        d_ip = to_dev(b"".join(ips))
        d_dg, d_st = dev_fill(N * hl, 0xEE), dev_fill(N, 7)
        sync()
        ctx.digest_msgs_dev(ht, N, d_msgs.data_ptr(), len(packed), d_offs.data_ptr(), d_dg.data_ptr(), d_st.data_ptr(), cp,
                            d_ip.data_ptr() if ipl else None, ipl, ipl)
        sync()
        assert from_dev(d_st, N) == bytes(N) and from_dev(d_dg, N * hl) == b"".join(want[name][i] for i in idxs), (name, cpl, ipl)
        if (cpl, ipl) == (0, 0):
            # the slot kernel on the same content, where a slot holds it
            short = [j for j in range(N) if len(msgs[j]) <= T.MAX_LEN]
            assert len(short) > 100
            slots = ctx.digest_slots(ht, T.pack_slots([msgs[j] for j in short], 4096), 4096)
            assert slots == b"".join(want[name][idxs[j]] for j in short), name


def test_n_zero_and_empty_messages(ctx, want):
    for name in ("SHA224", "SHA3_512", "STREEBOG256", "BASH384", "RIPEMD160"):
        ht = D.HASH_IDS[name]
        assert ctx.digest_msgs(ht, []) == (b"", b"")
        assert ctx.L.ec_digest_msgs_batch(ctx.h, ht, 0, None, None, None, 0, None, 0, 0, None, None) == 0
        assert ctx.L.ec_digest_msgs_batch_dev(ctx.h, ht, 0, None, 0, None, None, 0, None, 0, 0, None, None, None) == 0
        assert ctx.digest_msgs(ht, [b"", b"", b""]) == (want[name][0] * 3, bytes(3))
        assert D.cases(name)[0][0] == 0


def test_call_level_errors(ctx):
    offs = (C.c_uint64 * 2)(0, 1)
    out = C.create_string_buffer(64)
    L, h = ctx.L, ctx.h
    for ht in M.NOT_SERVED:
        assert L.ec_digest_msgs_batch(h, ht, 1, b"a", offs, None, 0, None, 0, 0, out, None) == -1
        assert b"hash_type" in L.ecamd_last_error()
    assert L.ec_digest_msgs_batch(h, 2, 1, b"a", offs, bytes(257), 257, None, 0, 0, out, None) == -1
    assert L.ec_digest_msgs_batch(h, 2, 1, b"a", offs, None, 0, bytes(257), 257, 257, out, None) == -1
    assert L.ec_digest_msgs_batch(h, 2, 1, b"a", offs, None, 3, None, 0, 0, out, None) == -1
    assert L.ec_digest_msgs_batch(h, 2, 1, b"a", offs, None, 0, None, 3, 3, out, None) == -1
    assert L.ec_digest_msgs_batch(h, 2, 1, b"a", offs, None, 0, b"abc", 3, 2, out, None) == -1
    assert L.ec_digest_msgs_batch(h, 2, 1, b"a", None, None, 0, None, 0, 0, out, None) == -1
    assert L.ec_digest_msgs_batch(h, 2, 1, b"a", offs, None, 0, None, 0, 0, None, None) == -1
    assert L.ec_digest_msgs_batch(h, 2, 1, None, offs, None, 0, None, 0, 0, out, None) == -1
    assert L.ec_digest_msgs_batch(None, 2, 1, b"a", offs, None, 0, None, 0, 0, out, None) == -1


@pytest.mark.parametrize("name", ["SHA256", "SHA3_256", "SHA512_224", "STREEBOG512", "BASH512"])
def test_unusable_items(ctx, name):
    """decreasing offsets, and an end behind the msgs_len that is passed: status 1, a zero digest, the neighbours untouched.  Every
    offset points inside the tensor that is allocated (40 octets; msgs_len says 32)."""
    ht, hl = D.HASH_IDS[name], D.HASH_SIZES[name]
    arr = D.stream("digest_msgs/unusable", 40)
    offs = [0, 10, 5, 20, 30, 40]
    def h(x):
        return hash_of(name, x)
    exp = h(arr[0:10]) + bytes(hl) + h(arr[5:20]) + h(arr[20:30]) + bytes(hl)
    d_msgs, d_offs, d_dg, d_st = to_dev(arr, 4), to_dev(u64s(offs), 8), dev_fill(5 * hl, 0xEE), dev_fill(5, 7)
    sync()
    ctx.digest_msgs_dev(ht, 5, d_msgs.data_ptr(), 32, d_offs.data_ptr(), d_dg.data_ptr(), d_st.data_ptr())
    sync()
    assert from_dev(d_st, 5) == bytes([0, 1, 0, 0, 1]) and from_dev(d_dg, 5 * hl) == exp
    # the host form judges by offsets[n] = 40: the last item is usable there
    out, st = C.create_string_buffer(5 * hl), C.create_string_buffer(5)
    assert ctx.L.ec_digest_msgs_batch(ctx.h, ht, 5, arr, (C.c_uint64 * 6)(*offs), None, 0, None, 0, 0, out, st) == 0
    assert st.raw == bytes([0, 1, 0, 0, 0]) and out.raw == exp[:4 * hl] + h(arr[30:40])
    # ... and an offset above it makes the items on both sides of it unusable
    offs2 = [0, 10, 50, 20, 30, 40]
    assert ctx.L.ec_digest_msgs_batch(ctx.h, ht, 5, arr, (C.c_uint64 * 6)(*offs2), None, 0, None, 0, 0, out, st) == 0
    assert st.raw == bytes([0, 1, 1, 0, 0]) and out.raw == h(arr[0:10]) + bytes(2 * hl) + h(arr[20:30]) + h(arr[30:40])


def proto_batch(curve, name, fx):
    """130 verification items -- per message the honest signature, a flipped signature bit, a flipped message bit, walked round -- and the
    six signing items"""
    rec = fx["proto"]["%s/%s" % (curve, name)]
    items = [D.proto_item(curve, name, i) for i in range(len(D.PROTO_LENS))]
    sigs = [bytes.fromhex(s) for s in rec["sigs"]]
    ver = []
    for (priv, pub, msg), sig, v in zip(items, sigs, rec["verdicts"]):
        ver += [(pub, sig, msg, v[0]), (pub, D.flip_sig(sig), msg, v[1]), (pub, sig, D.flip_msg(msg), v[2])]
    return items, sigs, [ver[k % len(ver)] for k in range(N)]


@pytest.mark.parametrize("curve,name", D.PROTO)
def test_ecdsa_verify_msgs(ctx, fx, curve, name):
    cv = ctx.curve(curve)
    try:
        _, _, ver = proto_batch(curve, name, fx)
        pubs, sigs, msgs = b"".join(v[0] for v in ver), b"".join(v[1] for v in ver), [v[2] for v in ver]
        exp = bytes(0 if v[3] == 0 else 1 for v in ver)
        assert 0 in exp and 1 in exp
        ht = D.HASH_IDS[name]
        assert cv.ecdsa_verify_msg_list(ht, pubs, sigs, msgs) == exp
        assert capped(ctx, 50000, 64, lambda: cv.ecdsa_verify_msg_list(ht, pubs, sigs, msgs)) == exp
        # the _dev form, with the first item's offsets decreasing: result 1 for it, whatever its signature says
        offs = offsets_of(map(len, msgs))
        offs[0] = offs[1] + 1
        packed = b"".join(msgs)
        assert exp[0] == 0 and offs[0] <= len(packed)
        d_pub, d_sig, d_msgs, d_offs, d_res = to_dev(pubs), to_dev(sigs), to_dev(packed, 4), to_dev(u64s(offs), 8), dev_fill(N, 7)
        sync()
        cv.ecdsa_verify_msgs_dev(ht, N, d_pub.data_ptr(), d_sig.data_ptr(), d_msgs.data_ptr(), len(packed), d_offs.data_ptr(), d_res.data_ptr())
        sync()
        assert from_dev(d_res, N) == b"\x01" + exp[1:]
    finally:
        cv.free()


@pytest.mark.parametrize("curve,name", D.PROTO)
def test_decdsa_sign_msgs(ctx, fx, curve, name):
    cv = ctx.curve(curve)
    try:
        items, sigs, _ = proto_batch(curve, name, fx)
        ht, ql = D.HASH_IDS[name], O.qlen(curve)
        privs = b"".join(items[k % 6][0] for k in range(N))
        msgs = [items[k % 6][2] for k in range(N)]
        exp = b"".join(sigs[k % 6] for k in range(N))
        for secret in (False, True):
            ctx.set_secret_scalars(secret)
            assert cv.decdsa_sign_msgs(ht, privs, msgs) == (exp, bytes(N)), (curve, name, secret)
        assert capped(ctx, 50000, 64, lambda: cv.decdsa_sign_msgs(ht, privs, msgs)) == (exp, bytes(N))
        # the _dev form; the last item ends behind the msgs_len that is passed (the tensor holds all of it): status 1 with zero bytes
        offs = offsets_of(map(len, msgs[:6]))
        packed = b"".join(msgs[:6])
        d_priv, d_msgs, d_offs = to_dev(privs[:6 * ql]), to_dev(packed, 4), to_dev(u64s(offs), 8)
        d_sig, d_st = dev_fill(6 * 2 * ql, 0xEE), dev_fill(6, 7)
        sync()
        cv.decdsa_sign_msgs_dev(ht, 6, d_priv.data_ptr(), d_msgs.data_ptr(), len(packed) - 1, d_offs.data_ptr(), d_sig.data_ptr(), d_st.data_ptr())
        sync()
        assert from_dev(d_st, 6) == bytes([0, 0, 0, 0, 0, 1])
        assert from_dev(d_sig, 12 * ql) == exp[:10 * ql] + bytes(2 * ql)
    finally:
        ctx.set_secret_scalars(False)
        assert ctx.L.ecamd_ctx_wipe_scratch(ctx.h) == 0
        cv.free()


def test_streebog_is_refused_in_secret_scalar_mode(ctx):
    cv = ctx.curve("SECP256R1")
    try:
        priv = (5).to_bytes(32, "big")
        ctx.set_secret_scalars(True)
        for ht in (13, 14):
            with pytest.raises(libecc_amd.EcamdError, match="Streebog"):
                cv.decdsa_sign_msgs(ht, priv, [b"abc"])
        # digests are public: served in this mode
        assert ctx.digest_msgs(13, [b"abc"])[1] == b"\0"
        ctx.set_secret_scalars(False)
        sig, st = cv.decdsa_sign_msgs(13, priv, [b"abc"])
        assert st == b"\0" and len(sig) == 64 and sig != bytes(64)
    finally:
        ctx.set_secret_scalars(False)
        cv.free()


KCDSA = [c for c in K.load_fixture() if c["alg"] == "ECKCDSA"]


@pytest.mark.parametrize("case", KCDSA, ids=[c["id"] for c in KCDSA])
def test_eckcdsa_composition_on_the_published_cases(ctx, case):
    """item_prefix = z (the first BLOCK octets of Yx || Yy, zero-padded), the digests h = H(z || m) stay on the device and go to
    ec_sig_hashed_verify_ht_batch_dev on the same stream: the recorded verdicts"""
    import torch
    hx = bytes.fromhex
    curve, name = case["curve"], case["hash"]
    ht, hl, blk = K.HASH_IDS[name], K.HSIZE[name], M.BLOCKS[name]
    vs = case["variants"]
    items = [vs[i % len(vs)] for i in range(N)]
    exp = bytes(0 if v["ret"] == 0 else 1 for v in items)
    assert 0 in exp and 1 in exp
    pubs, sigs, msgs = ([hx(v[f]) for v in items] for f in ("pub", "sig", "msg"))
    z = b"".join((p + bytes(blk))[:blk] for p in pubs)
    packed = b"".join(msgs)
    cv = ctx.curve(curve)
    try:
        stream = torch.cuda.Stream(device=torch.device("cuda:0"))
        d_pub, d_sig, d_z = to_dev(b"".join(pubs)), to_dev(b"".join(sigs)), to_dev(z)
        d_msgs, d_offs = to_dev(packed, 4), to_dev(u64s(offsets_of(map(len, msgs))), 8)
        d_h, d_res = dev_fill(N * hl, 0xEE), dev_fill(N, 7)
        sync()
        ctx.digest_msgs_dev(ht, N, d_msgs.data_ptr(), len(packed), d_offs.data_ptr(), d_h.data_ptr(), None, b"", d_z.data_ptr(), blk, blk,
                            stream.cuda_stream)
        cv.sig_hashed_verify_ht_dev(K.ALGS["ECKCDSA"], ht, N, d_pub.data_ptr(), d_sig.data_ptr(), d_h.data_ptr(), hl, d_res.data_ptr(),
                                    stream.cuda_stream)
        sync()
        assert from_dev(d_res, N) == exp, case["id"]
    finally:
        cv.free()
