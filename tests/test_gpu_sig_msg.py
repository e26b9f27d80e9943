"""GPU tests of ECGDSA / ECRDSA / SM2 from messages (ec_sig_verify_msg_batch, ec_sig_sign_msg_batch, ec_hash_slots_batch and their
_dev forms): SM3 and Streebog on the device against the recorded reference answers of tests/golden/sig_msg.json, chunk and wave edges,
every recorded verify and sign item, random batches against the digest-level calls fed with host digests, secret-scalar mode, the
_dev forms, SM2's key supplied or derived, the per-item rejections and the call-level errors.  All comparisons are exact bytes."""
import ctypes as C

import numpy as np
import pytest

import oracles as O
import sigfam_ref as S
import sigmsg_ref as M

pytestmark = pytest.mark.gpu
BATCH_COMBOS = M.COMBOS


@pytest.fixture(scope="module")
def fx():
    return M.load_fixture()


@pytest.fixture(scope="module")
def ctx():
    import libecc_amd
    c = libecc_amd.Context(0)
    yield c
    c.close()


def groups(items, *keys):
    out = {}
    for i in items:
        out.setdefault(tuple(i[k] for k in keys), []).append(i)
    return out


def blank_of(alg_name, hash_name):
    return M.HASH_SIZES[hash_name] if alg_name == "SM2" else 0


def test_hash_kats(ctx, fx):
    for (name,), items in groups(fx["hash"], "hash").items():
        msgs = [bytes.fromhex(i["msg"]) for i in items]
        got = ctx.hash_slots(M.HASH_IDS[name], M.pack_slots(msgs, 4092), 4092)
        assert got.hex() == "".join(i["digest"] for i in items), name


@pytest.mark.parametrize("name", ["SM3", "STREEBOG256", "STREEBOG512"])
def test_hash_mixed_lengths_chunks_and_wave_edges(ctx, fx, name):
    kat = {len(i["msg"]) // 2: i["digest"] for i in fx["hash"] if i["hash"] == name and i["msg"][:2] != "ff"}
    lens = [M.KAT_LENGTHS[i % len(M.KAT_LENGTHS)] for i in range(130)]
    slots = M.pack_slots([M.counting(n) for n in lens], 4092)
    exp = "".join(kat[n] for n in lens)
    hl = M.HASH_SIZES[name]
    ctx.set_max_chunk(64)       # three chunks
    try:
        assert ctx.hash_slots(M.HASH_IDS[name], slots, 4092).hex() == exp
    finally:
        ctx.set_max_chunk(1 << 20)
    for n in (1, 63, 64, 65):
        assert ctx.hash_slots(M.HASH_IDS[name], slots[:n * 4092], 4092).hex() == exp[:2 * hl * n], n


def test_hash_dev_form_and_overlong_slot(ctx, fx):
    import torch
    dev = torch.device("cuda:0")
    for name in ("SM3", "STREEBOG256", "STREEBOG512"):
        items = [i for i in fx["hash"] if i["hash"] == name and len(i["msg"]) // 2 <= 129]
        msgs = [bytes.fromhex(i["msg"]) for i in items]
        slots = bytearray(M.pack_slots(msgs, 136))
        slots[136:140] = (133).to_bytes(4, "little")       # item 1: 4 + 133 > 136
        hl, n = M.HASH_SIZES[name], len(items)
        d_in = torch.frombuffer(bytearray(slots), dtype=torch.uint8).to(dev)
        d_out = torch.full((n * hl,), 0xAA, dtype=torch.uint8, device=dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        ctx.hash_slots_dev(M.HASH_IDS[name], n, d_in.data_ptr(), 136, d_out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        got = bytes(d_out.cpu().numpy())
        exp = b"".join(bytes(hl) if j == 1 else bytes.fromhex(i["digest"]) for j, i in enumerate(items))
        assert got == exp, name
        assert bytes(d_in.cpu().numpy()) == bytes(slots)


def verify_call(ctx, curve, alg_name, hash_name, items, ident):
    cv = ctx.curve(curve)
    try:
        msgs = [bytes.fromhex(i["msg"]) for i in items]
        blank = blank_of(alg_name, hash_name)
        stride = M.stride_for(msgs, blank)
        slots = M.pack_slots(msgs, stride, blank)
        before = bytes(slots)
        got = cv.sig_verify_msg(S.SCHEMES[alg_name], M.HASH_IDS[hash_name], b"".join(bytes.fromhex(i["pub"]) for i in items),
                                b"".join(bytes.fromhex(i["sig"]) for i in items), slots, stride, ident)
        assert slots == before
        return got
    finally:
        cv.free()


def test_every_recorded_verify_item(ctx, fx):
    for (curve, alg_name, hash_name, ident), items in groups(fx["verify"], "curve", "alg", "hash", "id").items():
        got = verify_call(ctx, curve, alg_name, hash_name, items, bytes.fromhex(ident))
        exp = bytes(0 if i["ret"] == 0 else 1 for i in items)
        assert got == exp, (curve, alg_name, hash_name, [i["family"] for j, i in enumerate(items) if got[j] != exp[j]])


def sign_inputs(curve, items):
    ql = O.qlen(curve)
    top = (1 << (8 * ql)) - 1
    xs = b"".join(min(int(i["x"], 16), top).to_bytes(ql, "big") for i in items)
    ks = b"".join(min(int(i["k"], 16), top).to_bytes(ql, "big") for i in items)
    sigs = b"".join(bytes.fromhex(i["sig"]) if i["ret"] == 0 else bytes(2 * ql) for i in items)
    return xs, ks, sigs, bytes(0 if i["ret"] == 0 else 1 for i in items)


def test_every_recorded_sign_item(ctx, fx):
    for (curve, alg_name, hash_name, ident), items in groups(fx["sign"], "curve", "alg", "hash", "id").items():
        cv = ctx.curve(curve)
        try:
            xs, ks, sigs, st = sign_inputs(curve, items)
            msgs = [bytes.fromhex(i["msg"]) for i in items]
            blank = blank_of(alg_name, hash_name)
            stride = M.stride_for(msgs, blank)
            got = cv.sig_sign_msg(S.SCHEMES[alg_name], M.HASH_IDS[hash_name], xs, ks, M.pack_slots(msgs, stride, blank), stride,
                                  bytes.fromhex(ident))
            assert got[1] == st, (curve, alg_name, hash_name, [i["family"] for j, i in enumerate(items) if got[1][j] != st[j]])
            assert got[0] == sigs, (curve, alg_name, hash_name)
        finally:
            cv.free()


def random_batch(ctx, curve, alg, hash_name, n, seed, ident):
    """n keys, nonces and messages of 0 .. 70 octets with the host digests the digest-level calls take.  The public keys come from the
    library's own fixed-base multiplication (tests/test_gpu_parity.py holds it against the reference): Python's would take most of the
    test's time on a 512-bit curve."""
    rng = np.random.default_rng(seed)
    q, ql, cl = O.CURVES[curve]["q"], O.qlen(curve), O.clen(curve)
    xs = [1 + S.rand_int(rng, q - 2) for _ in range(n)]
    cv = ctx.curve(curve)
    try:
        pts, st = cv.scalar_mult(b"".join((pow(x, -1, q) if alg == S.ECGDSA else x).to_bytes(ql, "big") for x in xs))
    finally:
        cv.free()
    assert bytes(st) == bytes(n) and len(pts) == 2 * cl * n
    pubs = [bytes(pts[2 * cl * i:2 * cl * (i + 1)]) for i in range(n)]
    assert pubs[0] == S.pt_bytes(curve, S.pub_point(curve, alg, xs[0]))
    msgs = [rng.integers(0, 256, size=int(rng.integers(0, 71)), dtype=np.uint8).tobytes() for _ in range(n)]
    with M.swapped(M.shim_hash, hash_name, ident):
        dgs = [S.digest_for(curve, alg, hash_name, pubs[i], msgs[i]) for i in range(n)]
    ks = [1 + S.rand_int(rng, q - 1) for _ in range(n)]
    return (b"".join(x.to_bytes(ql, "big") for x in xs), b"".join(k.to_bytes(ql, "big") for k in ks), b"".join(pubs), msgs, b"".join(dgs))


_BATCHES = {}


def batch_for(ctx, combo):
    if combo not in _BATCHES:
        alg_name, hash_name, curve = combo
        _BATCHES[combo] = random_batch(ctx, curve, S.SCHEMES[alg_name], hash_name, 256, 4242, b"signer@example.org")
    return _BATCHES[combo]


def to_dev(*arrays):
    import torch
    return [torch.frombuffer(bytearray(a), dtype=torch.uint8).to(torch.device("cuda:0")) for a in arrays]


@pytest.mark.parametrize("combo", BATCH_COMBOS, ids=["-".join(c) for c in BATCH_COMBOS])
def test_random_batch_equals_digest_level_calls(ctx, combo):
    import torch
    alg_name, hash_name, curve = combo
    alg, ht, hl = S.SCHEMES[alg_name], M.HASH_IDS[hash_name], M.HASH_SIZES[hash_name]
    ident = b"signer@example.org" if alg_name == "SM2" else None
    xs, ks, pubs, msgs, dgs = batch_for(ctx, combo)
    n = len(msgs)
    blank = blank_of(alg_name, hash_name)
    stride = M.stride_for(msgs, blank)
    slots = M.pack_slots(msgs, stride, blank)
    cv = ctx.curve(curve)
    try:
        exp = cv.sig_sign(alg, xs, ks, dgs, hl)
        assert exp[1] == bytes(n)
        got = cv.sig_sign_msg(alg, ht, xs, ks, slots, stride, ident, pubs if alg_name == "SM2" else None)
        assert got == exp
        if alg_name == "SM2":      # Y = [x]G on the device
            assert cv.sig_sign_msg(alg, ht, xs, ks, slots, stride, ident, None) == exp
        ctx.set_secret_scalars(True)
        try:
            assert cv.sig_sign_msg(alg, ht, xs, ks, slots, stride, ident, None) == exp
        finally:
            ctx.set_secret_scalars(False)
        # verification: the honest signatures, every fourth with another item's message
        sigs = exp[0]
        vmsgs = [msgs[(i + 1) % n] if i % 4 == 3 else msgs[i] for i in range(n)]
        with M.swapped(M.shim_hash, hash_name, ident or b""):
            ql2, pl = 2 * cv.qlen, 2 * cv.clen
            vdgs = b"".join(S.digest_for(curve, alg, hash_name, pubs[i * pl:(i + 1) * pl], vmsgs[i]) for i in range(n))
        vslots = M.pack_slots(vmsgs, stride, blank)
        vexp = cv.sig_verify(alg, pubs, sigs, vdgs, hl)
        assert vexp.count(0) >= n // 2 and vexp.count(1) >= n // 8
        assert cv.sig_verify_msg(alg, ht, pubs, sigs, vslots, stride, ident) == vexp
        # the _dev forms, in two chunks
        ctx.set_max_chunk(192)
        try:
            d = to_dev(xs, ks, pubs, slots, vslots, sigs)
            dsig = torch.full((ql2 * n,), 0xAA, dtype=torch.uint8, device=d[0].device)
            dst = torch.full((n,), 0xAA, dtype=torch.uint8, device=d[0].device)
            dres = torch.full((n,), 0xAA, dtype=torch.uint8, device=d[0].device)
            stream = torch.cuda.Stream(device=d[0].device)
            torch.cuda.synchronize()
            cv.sig_sign_msg_dev(alg, ht, n, d[0].data_ptr(), d[2].data_ptr() if alg_name == "SM2" else None, d[1].data_ptr(), d[3].data_ptr(),
                                stride, ident, dsig.data_ptr(), dst.data_ptr(), stream.cuda_stream)
            cv.sig_verify_msg_dev(alg, ht, n, d[2].data_ptr(), d[5].data_ptr(), d[4].data_ptr(), stride, ident, dres.data_ptr(),
                                  stream.cuda_stream)
            stream.synchronize()
            assert (bytes(dsig.cpu().numpy()), bytes(dst.cpu().numpy())) == exp
            assert bytes(dres.cpu().numpy()) == vexp
            assert bytes(d[3].cpu().numpy()) == slots and bytes(d[4].cpu().numpy()) == vslots
        finally:
            ctx.set_max_chunk(1 << 20)
    finally:
        cv.free()


@pytest.mark.parametrize("combo", [M.COMBOS[0], M.COMBOS[2]], ids=["SM2-SM3", "ECRDSA-STREEBOG256"])
def test_per_item_rejections_stay_with_their_item(ctx, combo):
    alg_name, hash_name, curve = combo
    alg, ht, hl = S.SCHEMES[alg_name], M.HASH_IDS[hash_name], M.HASH_SIZES[hash_name]
    ident = b"signer@example.org" if alg_name == "SM2" else None
    xs, ks, pubs, msgs, dgs = batch_for(ctx, combo)
    n, blank = 8, blank_of(alg_name, hash_name)
    cv = ctx.curve(curve)
    try:
        ql, pl = cv.qlen, 2 * cv.clen
        xs, ks, pubs, msgs = xs[:n * ql], ks[:n * ql], bytearray(pubs[:n * pl]), msgs[:n]
        stride = M.stride_for(msgs, blank)
        good = M.pack_slots(msgs, stride, blank)
        sigs, st = cv.sig_sign_msg(alg, ht, xs, ks, good, stride, ident, bytes(pubs))
        assert st == bytes(n)
        slots = bytearray(good)
        slots[1 * stride:1 * stride + 4] = (stride - 3).to_bytes(4, "little")          # too long for its stride
        bad = {1}
        if blank:
            slots[3 * stride:3 * stride + 4] = (blank - 1).to_bytes(4, "little")        # shorter than its blank
            bad.add(3)
        pubs[5 * pl + pl - 1] ^= 1                                                       # off the curve
        before = bytes(slots)
        res = cv.sig_verify_msg(alg, ht, bytes(pubs), sigs, bytes(slots), stride, ident)
        assert res == bytes(1 if i in bad | {5} else 0 for i in range(n))
        assert bytes(slots) == before
        s2, st2 = cv.sig_sign_msg(alg, ht, xs, ks, bytes(slots), stride, ident, bytes(pubs))
        sbad = bad | ({5} if alg_name == "SM2" else set())      # only SM2's signing reads the key
        assert st2 == bytes(1 if i in sbad else 0 for i in range(n))
        for i in range(n):
            assert s2[i * 2 * ql:(i + 1) * 2 * ql] == (bytes(2 * ql) if i in sbad else sigs[i * 2 * ql:(i + 1) * 2 * ql]), i
        if blank:      # a stride that cannot hold the blank: every item
            tiny = M.pack_slots([b""] * n, 4)
            assert cv.sig_verify_msg(alg, ht, bytes(pubs), sigs, tiny, 4, ident) == bytes([1] * n)
            assert cv.sig_sign_msg(alg, ht, xs, ks, tiny, 4, ident) == (bytes(2 * ql * n), bytes([1] * n))
    finally:
        cv.free()


def test_call_level_errors(ctx):
    import libecc_amd
    cv = ctx.curve("SM2P256V1")
    try:
        ql, pl = cv.qlen, 2 * cv.clen
        slots = M.pack_slots([b"m"], 40, 32)
        args = (bytes(pl), bytes(2 * ql), slots, 40)
        for alg, ht, ident, idl, what in ((S.SM2, 5, b"id", 2, "hash_type"), (1, 11, b"id", 2, "alg"), (S.SM2, 11, bytes(1025), 1025, "id_len"),
                                          (S.SM2, 11, None, 4, "NULL"), (S.SM2, 13, b"id", 2, "Z")):
            res, so, sto = C.create_string_buffer(1), C.create_string_buffer(2 * ql), C.create_string_buffer(1)
            rc = ctx.L.ec_sig_verify_msg_batch(ctx.h, cv.h, alg, ht, 1, args[0], args[1], args[2], args[3], ident, idl, res)
            assert rc == -1 and what in ctx.L.ecamd_last_error().decode(), what
            rc = ctx.L.ec_sig_sign_msg_batch(ctx.h, cv.h, alg, ht, 1, bytes(ql), None, bytes(ql), args[2], args[3], ident, idl, so, sto)
            assert rc == -1 and what in ctx.L.ecamd_last_error().decode(), what
        with pytest.raises(libecc_amd.EcamdError):
            ctx.hash_slots(5, slots, 40)
        with pytest.raises(libecc_amd.EcamdError):
            ctx.hash_slots(11, slots[:38] + bytes(4), 42)
        assert cv.sig_verify_msg(S.SM2, 11, b"", b"", b"", 40, b"id") == b""      # n = 0
        # id and id_len are ignored unless alg is SM2
        rc = ctx.L.ec_sig_verify_msg_batch(ctx.h, cv.h, S.ECRDSA, 13, 1, args[0], args[1], args[2], args[3], None, 5000, C.create_string_buffer(1))
        assert rc == 0
    finally:
        cv.free()
