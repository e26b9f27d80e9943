"""ec_eddsa_verify_msgs_batch, ec_eddsa_verify_msgs_all_batch and ec_eddsa_sign_msgs_batch on the device against tests/golden/eddsa_msgs.json,
the unmodified reference's keys, signatures and verdicts, for all five variants.  A batch has 130 items (two full waves and a tail of
two) under ONE context; the fixture's cases of that context and their damaged variants are walked round and round, so the 70 001-octet
message sits among short ones, the lanes of a wave diverge and message starts fall at every residue mod 8.  Each batch runs as one
chunk and at max_chunk 64; the host forms also under a byte cap that makes the long message a piece of its own.
The library's stream is not torch's: device buffers are kept until the test has synchronised (see test_gpu_sig_kats.py)."""
import ctypes as C
import os

import pytest

import libecc_amd
import eddsa_sign_ref as E
import eddsa_msgs_ref as D

pytestmark = pytest.mark.gpu
N = 130
CAP_ENV = "ECAMD_MSGS_CHUNK_BYTES"
HOST_MODES = [(0, 1 << 20), (0, 64), (50000, 1 << 20)]   # (byte cap, max_chunk)
DEV_CHUNKS = [1 << 20, 64]


@pytest.fixture(scope="module")
def ctx():
    c = libecc_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def curves(ctx):
    return {False: ctx.curve("WEI25519"), True: ctx.curve("WEI448")}


@pytest.fixture(scope="module")
def groups():
    """{alg: [(adata, [fixture item])]}: the cases of one alg by context"""
    fx = D.load_fixture()
    return {alg: list(D.by_context(D.fixture_items(fx, alg)).items()) for alg in D.ALGS}


STEP = 5   # the cases are walked five apart (coprime to every group's size): neighbouring lanes differ widely in length


def pick(items, j):
    return items[(STEP * j) % len(items)]


def verify_batch(items):
    """130 (pub, sig, msg, result, kind) cycling the cases and, per case, its variants"""
    out = []
    for j in range(N):
        var = pick(items, j)["variants"]
        kind, pub, sig, msg, verdict = var[j % len(var)]
        out.append((pub, sig, msg, 0 if verdict == 0 else 1, kind))
    return out


def sign_batch(items):
    return [pick(items, j) for j in range(N)]


def to_dev(bs, pad_to=1):
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


def offsets_of(msgs):
    offs, pos = [0], 0
    for m in msgs:
        pos += len(m)
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


def alen(adata):
    return len(adata) if adata is not None else 0


def verify_dev(cv, alg, adata, pubs, sigs, packed, offs, msgs_len=None):
    n = len(offs) - 1
    d_pub, d_sig, d_msgs, d_offs, d_res = to_dev(pubs), to_dev(sigs), to_dev(packed, 4), to_dev(u64s(offs), 8), dev_fill(n, 7)
    sync()
    cv.eddsa_verify_msg_list_dev(alg, n, d_pub.data_ptr(), d_sig.data_ptr(), adata, d_msgs.data_ptr(), len(packed) if msgs_len is None else msgs_len,
                                 d_offs.data_ptr(), d_res.data_ptr())
    sync()
    return from_dev(d_res, n)


def sign_dev(cv, alg, adata, sks, pubs, packed, offs, msgs_len=None):
    n, kl = len(offs) - 1, E.klen(alg)
    d_sk, d_pub = to_dev(sks), (to_dev(pubs) if pubs is not None else None)
    d_msgs, d_offs = to_dev(packed, 4), to_dev(u64s(offs), 8)
    d_sig, d_po, d_st = dev_fill(2 * kl * n, 0xEE), dev_fill(kl * n, 0xEE), dev_fill(n, 7)
    sync()
    cv.eddsa_sign_msg_list_dev(alg, n, d_sk.data_ptr(), d_pub.data_ptr() if pubs is not None else None, adata, d_msgs.data_ptr(),
                               len(packed) if msgs_len is None else msgs_len, d_offs.data_ptr(), d_sig.data_ptr(), d_po.data_ptr(), d_st.data_ptr())
    sync()
    return from_dev(d_sig, 2 * kl * n), from_dev(d_po, kl * n), from_dev(d_st, n)


def sign_host_raw(cv, alg, adata, sks, pubs, packed, offs):
    """the host form with offsets of the caller's making"""
    n, kl = len(offs) - 1, E.klen(alg)
    sigs, po, st = C.create_string_buffer(2 * kl * n), C.create_string_buffer(kl * n), C.create_string_buffer(n)
    o = (C.c_uint64 * (n + 1))(*offs)
    assert cv.L.ec_eddsa_sign_msgs_batch(cv.ctx.h, cv.h, alg, n, sks, pubs, adata, alen(adata), packed, o, sigs, po, st) == 0, cv.L.ecamd_last_error()
    return sigs.raw, po.raw, st.raw


def verify_host_raw(cv, alg, adata, pubs, sigs, packed, offs):
    n = len(offs) - 1
    res = C.create_string_buffer(n)
    o = (C.c_uint64 * (n + 1))(*offs)
    assert cv.L.ec_eddsa_verify_msgs_batch(cv.ctx.h, cv.h, alg, n, pubs, sigs, adata, alen(adata), packed, o, res) == 0, cv.L.ecamd_last_error()
    return res.raw


@pytest.mark.parametrize("alg", D.ALGS)
def test_verification_gives_the_reference_verdicts(ctx, curves, groups, alg):
    cv = curves[E.is448(alg)]
    assert len(groups[alg]) == (3 if E.takes_ctx(alg) else 1)
    seen_long = False
    for g, (adata, items) in enumerate(groups[alg]):
        batch = verify_batch(items)
        pubs, sigs, msgs = b"".join(b[0] for b in batch), b"".join(b[1] for b in batch), [b[2] for b in batch]
        want = bytes(b[3] for b in batch)
        offs = offsets_of(msgs)
        assert {b[4] for b in batch} == set(D.KINDS) and 0 in want and 1 in want
        assert {o % 8 for o in offs[:-1]} == set(range(8))
        seen_long |= any(len(m) == D.LONG for m in msgs)
        # the context that carries the long message runs every mode, the others one each in turn
        full = any(len(m) == D.LONG for m in msgs)
        for cap, chunk in (HOST_MODES if full else [HOST_MODES[g % 3]]):
            got = capped(ctx, cap, chunk, lambda: cv.eddsa_verify_msg_list(alg, pubs, sigs, msgs, adata))
            assert got == want, (alg, alen(adata), cap, chunk, [j for j in range(N) if got[j] != want[j]][:8])
        for chunk in (DEV_CHUNKS if full else [DEV_CHUNKS[g % 2]]):
            got = capped(ctx, 0, chunk, lambda: verify_dev(cv, alg, adata, pubs, sigs, b"".join(msgs), offs))
            assert got == want, (alg, alen(adata), chunk, [j for j in range(N) if got[j] != want[j]][:8])
    assert seen_long


@pytest.mark.parametrize("alg", D.ALGS)
def test_signing_gives_the_reference_bytes(ctx, curves, groups, alg):
    cv = curves[E.is448(alg)]
    for g, (adata, items) in enumerate(groups[alg]):
        batch = sign_batch(items)
        sks, pubs, msgs = b"".join(b["sk"] for b in batch), b"".join(b["pub"] for b in batch), [b["msg"] for b in batch]
        want = b"".join(b["sig"] for b in batch)
        full = any(len(m) == D.LONG for m in msgs)
        for k, (cap, chunk) in enumerate(HOST_MODES if full else [HOST_MODES[g % 3]]):
            given = pubs if k % 2 == 0 else None     # the keys supplied, and derived on the device
            sg, po, st = capped(ctx, cap, chunk, lambda: cv.eddsa_sign_msg_list(alg, sks, given, msgs, adata))
            assert st == bytes(N) and sg == want and po == pubs, (alg, alen(adata), cap, chunk, given is None)
        for k, chunk in enumerate(DEV_CHUNKS if full else [DEV_CHUNKS[g % 2]]):
            given = None if k % 2 == 0 else pubs
            sg, po, st = capped(ctx, 0, chunk, lambda: sign_dev(cv, alg, adata, sks, given, b"".join(msgs), offsets_of(msgs)))
            assert st == bytes(N) and sg == want and po == pubs, (alg, alen(adata), chunk, given is None)
        if full:
            try:
                ctx.set_secret_scalars(True)
                sg, po, st = capped(ctx, 0, 64, lambda: cv.eddsa_sign_msg_list(alg, sks, None, msgs, adata))
                assert st == bytes(N) and sg == want and po == pubs, (alg, "secret scalars, host")
                sg, po, st = sign_dev(cv, alg, adata, sks, pubs, b"".join(msgs), offsets_of(msgs))
                assert st == bytes(N) and sg == want and po == pubs, (alg, "secret scalars, dev")
            finally:
                ctx.set_secret_scalars(False)


@pytest.mark.parametrize("alg", D.ALGS)
def test_whole_batch_bit(ctx, curves, groups, alg):
    cv = curves[E.is448(alg)]
    adata, items = max(groups[alg], key=lambda g: len(g[1]))
    batch = sign_batch(items)
    kl = E.klen(alg)
    pubs, sigs, msgs = b"".join(b["pub"] for b in batch), b"".join(b["sig"] for b in batch), [b["msg"] for b in batch]
    damaged = bytearray(sigs)
    damaged[2 * kl * 77 + kl] ^= 1                       # a bit of S of item 77
    offs = offsets_of(msgs)
    bad_offs = list(offs)
    bad_offs[41] = offs[N] + 5                           # item 40 ends behind the array, item 41 begins there
    for chunk in DEV_CHUNKS:
        def run():
            out = [cv.eddsa_verify_msg_list_all(alg, pubs, sigs, msgs, adata), cv.eddsa_verify_msg_list_all(alg, pubs, bytes(damaged), msgs, adata)]
            d_pub, d_ok, d_bad = to_dev(pubs), to_dev(sigs), to_dev(bytes(damaged))
            d_msgs, d_offs, d_boffs, d_v = to_dev(b"".join(msgs), 4), to_dev(u64s(offs), 8), to_dev(u64s(bad_offs), 8), dev_fill(3, 7)
            sync()
            for k, (d_sig, d_o) in enumerate(((d_ok, d_offs), (d_bad, d_offs), (d_ok, d_boffs))):
                cv.eddsa_verify_msg_list_all_dev(alg, N, d_pub.data_ptr(), d_sig.data_ptr(), adata, d_msgs.data_ptr(), offs[N], d_o.data_ptr(),
                                                 d_v.data_ptr() + k)
            sync()
            return out, from_dev(d_v, 3)
        (honest, broken), dev = capped(ctx, 0, chunk, run)
        assert honest == (True, N) and broken == (False, 77), (alg, chunk)
        assert dev == bytes([1, 0, 0]), (alg, chunk, dev)
    # the host form with an unusable item: rejected, and the item counts for first_rejected
    ok, first = C.c_int(7), C.c_uint32(7)
    o = (C.c_uint64 * (N + 1))(*bad_offs)
    assert cv.L.ec_eddsa_verify_msgs_all_batch(cv.ctx.h, cv.h, alg, N, pubs, sigs, adata, alen(adata), b"".join(msgs), o, C.byref(ok), C.byref(first)) == 0
    assert (ok.value, first.value) == (0, 40)


@pytest.mark.parametrize("alg", D.ALGS)
def test_unusable_offsets_among_good_items(ctx, curves, groups, alg):
    cv = curves[E.is448(alg)]
    adata, items = max(groups[alg], key=lambda g: len(g[1]))
    kl = E.klen(alg)
    vb, sb = verify_batch(items), sign_batch(items)
    # an offset behind the array's end makes TWO unusable items: the one that ends there (offsets[i + 1] > the length) and the one
    # that begins there (offsets[i] > offsets[i + 1]); once in the first wave at an item the reference accepts, once across the
    # boundary of the second wave
    h = [j for j in range(2, 60) if vb[j][3] == 0][1]
    def spoil(offs):
        out = list(offs)
        out[h] = offs[N] + 5
        out[64] = offs[N] + (1 << 40)
        return out, (h - 1, h, 63, 64)
    # verification
    pubs, sigs, msgs = b"".join(b[0] for b in vb), b"".join(b[1] for b in vb), [b[2] for b in vb]
    offs, dead = spoil(offsets_of(msgs))
    want = bytes(1 if j in dead else vb[j][3] for j in range(N))
    assert want != bytes(b[3] for b in vb)
    for cap, chunk in HOST_MODES:
        assert capped(ctx, cap, chunk, lambda: verify_host_raw(cv, alg, adata, pubs, sigs, b"".join(msgs), offs)) == want, (alg, cap, chunk)
    for chunk in DEV_CHUNKS:
        assert capped(ctx, 0, chunk, lambda: verify_dev(cv, alg, adata, pubs, sigs, b"".join(msgs), offs)) == want, (alg, chunk)
    # ... and msgs_len of the _dev form below the last item's end: that item alone
    cut = offsets_of(msgs)
    assert len(msgs[N - 1]) > 0
    got = verify_dev(cv, alg, adata, pubs, sigs, b"".join(msgs), cut, msgs_len=cut[N] - 1)
    assert got == bytes(b[3] for b in vb[:N - 1]) + b"\x01"
    # signing
    sks, pubs, msgs = b"".join(b["sk"] for b in sb), b"".join(b["pub"] for b in sb), [b["msg"] for b in sb]
    offs, dead = spoil(offsets_of(msgs))
    want_sig = b"".join(bytes(2 * kl) if j in dead else sb[j]["sig"] for j in range(N))
    want_st = bytes(1 if j in dead else 0 for j in range(N))
    for cap, chunk in HOST_MODES[:2]:
        sg, po, st = capped(ctx, cap, chunk, lambda: sign_host_raw(cv, alg, adata, sks, None, b"".join(msgs), offs))
        assert (sg, st, po) == (want_sig, want_st, pubs), (alg, cap, chunk)
    sg, po, st = capped(ctx, 0, 64, lambda: sign_dev(cv, alg, adata, sks, pubs, b"".join(msgs), offs))
    assert (sg, st, po) == (want_sig, want_st, pubs), alg


@pytest.mark.parametrize("alg", D.ALGS)
def test_agreement_with_the_slot_calls(ctx, curves, groups, alg):
    """the same content of at most 4092 octets through the slot twins: ec_eddsa_sign_msg_batch for all five variants,
    ec_eddsa_verify_msg_batch (host-assembled dom2 || R || A || PH(M)) for the three it serves"""
    cv = curves[E.is448(alg)]
    kl = E.klen(alg)
    for adata, items in groups[alg]:
        short = [it for it in items if len(it["msg"]) <= 4092]
        assert len(short) >= len(items) - 2
        sb = [short[j % len(short)] for j in range(N)]
        sks, pubs, msgs = b"".join(b["sk"] for b in sb), b"".join(b["pub"] for b in sb), [b["msg"] for b in sb]
        slots, stride = cv.msg_slots(msgs)
        assert stride <= 4096
        ragged = cv.eddsa_sign_msg_list(alg, sks, None, msgs, adata)
        assert ragged == cv.eddsa_sign_msgs(alg, sks, None, adata, slots, stride), (alg, alen(adata))
        if not E.is448(alg):
            vb = [b for b in verify_batch(short) if len(b[2]) <= 3700]   # dom2 || R || A || M fits a slot
            pubs, sigs, msgs = b"".join(b[0] for b in vb), b"".join(b[1] for b in vb), [b[2] for b in vb]
            inputs = [E.dom(alg, adata) + b[1][:kl] + b[0] + E.PH(alg, b[2]) for b in vb]
            got = cv.eddsa_verify_msg_list(alg, pubs, sigs, msgs, adata)
            assert got == cv.eddsa_verify_msgs(pubs, sigs, inputs) == bytes(b[3] for b in vb), (alg, alen(adata))


def test_call_level_errors_and_empty_batches(ctx, curves):
    c25, c448 = curves[False], curves[True]
    L = c25.L
    o = (C.c_uint64 * 2)(0, 1)
    res = C.create_string_buffer(1)
    args = (1, bytes(32), bytes(64), None, 0, b"m", o, res)
    assert L.ec_eddsa_verify_msgs_batch(ctx.h, c25.h, 8, *args) == -1 and L.ec_eddsa_verify_msgs_batch(ctx.h, c25.h, 14, *args) == -1
    assert L.ec_eddsa_verify_msgs_batch(ctx.h, c25.h, 12, *args) == -1 and L.ec_eddsa_verify_msgs_batch(ctx.h, c448.h, 9, *args) == -1
    assert L.ec_eddsa_verify_msgs_batch(ctx.h, c25.h, 10, *args) == -1                      # EDDSA25519CTX without a context
    assert L.ec_eddsa_verify_msgs_batch(ctx.h, c25.h, 11, 1, bytes(32), bytes(64), bytes(256), 256, b"m", o, res) == -1
    assert L.ec_eddsa_verify_msgs_batch(ctx.h, c25.h, 9, 0, None, None, None, 0, None, None, None) == 0      # n = 0 touches nothing
    assert L.ec_eddsa_sign_msgs_batch(ctx.h, c25.h, 9, 0, None, None, None, 0, None, None, None, None, None) == 0
    ok = C.c_int(5)
    assert L.ec_eddsa_verify_msgs_all_batch(ctx.h, c25.h, 9, 0, bytes(32), bytes(64), None, 0, b"", o, C.byref(ok), None) == -1   # as the reference
    assert c25.eddsa_verify_msg_list(9, b"", b"", []) == b"" and c448.eddsa_sign_msg_list(12, b"", None, [], b"")[2] == b""
