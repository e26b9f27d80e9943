"""User-defined curves (ecamd_curve_from_params) at field sizes no built-in curve has, against the three references of
tests/user_curves.py: Python integers, the restatement oracle on the whole batch, and the recorded answers of the unmodified
reference (tests/golden/user_curves.json, bitlen(p) <= 521; the 544-bit curve rests on the first two).  Every comparison is
byte-exact.  tests/test_user_curves_host.py shows on the CPU that the references agree on these very batches."""
import os

import pytest

import oracles as O
import user_curves as U

pytestmark = pytest.mark.gpu

CURVES = U.load()
NAMES = sorted(CURVES)
_ORACLES = {}


def oracle(cv):
    if cv["name"] not in _ORACLES:
        _ORACLES[cv["name"]] = O.Oracle(cv)
    return _ORACLES[cv["name"]]


@pytest.fixture(scope="module")
def handles(gpu_ctx):
    """one handle per curve, made on first use: a curve the library refuses fails its tests (EcamdError), it is not skipped"""
    import libecc_amd
    made = {}

    def get(name):
        if name not in made:
            cv = CURVES[name]
            h = libecc_amd.Curve(gpu_ctx, params=U.params(cv))
            assert (h.clen, h.qlen, h.words) == (U.clen(cv), U.qlen(cv), U.words(cv))
            made[name] = h
        return made[name]
    yield get
    for h in made.values():
        h.free()


@pytest.mark.parametrize("name", NAMES)
def test_field_ops(handles, name):
    cv = CURVES[name]
    A, B = U.field_batch(cv)
    if name == "U544A":
        assert 4 * U.top_carry_count(cv, A, B) >= len(A)      # the Montgomery product's carry-word branch at 17 words is known to run
    h, o = handles(name), oracle(cv)
    for op in range(5):
        got = h.fp_op(op, A, B)
        assert got == U.py_field(cv, op, A, B), f"fp op {op} against Python"
        assert got == o.fp_op(op, A, B), f"fp op {op} against the oracle"


@pytest.mark.parametrize("name", NAMES)
def test_point_add_and_double(handles, name):
    cv = CURVES[name]
    A, B, exc = U.add_batch(cv)
    h, o = handles(name), oracle(cv)
    for key, got, exp in (("add", h.pt_add(A, B), o.pt_add(A, B)), ("dbl", h.pt_add(A), o.pt_add(A))):
        assert got == exp, key
        if cv["ref"] is not None:
            assert U.pack(U.ref_items(cv, key), got[1], got[0]) == cv["ref"][key], key
    st = h.pt_add(A, B)[1]
    assert st[exc:exc + 4] == b"\x00\x00\x00\x02" and st[exc + 4:exc + 9] == b"\x01" * 5      # T as an operand; the exceptional pairs
    cl = U.clen(cv)
    pairs = [(A[2 * cl * i:2 * cl * (i + 1)], B[2 * cl * i:2 * cl * (i + 1)]) for i in range(len(st))]
    assert h.pt_add(A, B) == U.py_add(cv, pairs)


@pytest.mark.parametrize("name", NAMES)
def test_scalar_mult(handles, name):
    cv = CURVES[name]
    h, o = handles(name), oracle(cv)
    for label, slen, sc, pts in U.smul_batches(cv):
        assert len(sc) // slen < 256
        got = h.scalar_mult(sc, pts, slen=slen)
        assert got == o.scalar_mult(sc, pts, slen=slen), label
        if cv["ref"] is not None:
            assert U.pack(U.ref_items(cv, label), got[1], got[0]) == cv["ref"]["smul"][label], label
    # a few of each against Python integers
    cl = U.clen(cv)
    label, slen, sc, pts = [b for b in U.smul_batches(cv) if b[0] == "var/q"][0]
    out, st = h.scalar_mult(sc, pts, slen=slen)
    idx = U.sample(len(st), 6)
    items = [(int.from_bytes(sc[slen * i:slen * (i + 1)], "big"), pts[2 * cl * i:2 * cl * (i + 1)]) for i in idx]
    assert U.py_smul(cv, items) == (b"".join(out[2 * cl * i:2 * cl * (i + 1)] for i in idx), bytes(st[i] for i in idx))


@pytest.mark.parametrize("name", ["U521B", "U544A", "X256A", "X512A"])
def test_fixed_base_above_the_comb_threshold(gpu_ctx, handles, name):
    """a fixed-base batch of at least the context's comb threshold (conftest.py lowers ECAMD_COMB_MIN_BATCH to 48 before the context
    is made): on the curves with a radix-2^29 unit the handle builds its generator comb for it and answers through it -- U521B is
    the generic unit of 521 bits, its table, comb and window kernels as a pipeline; U544A has no such unit and stays on the
    saturated-word kernel at the same batch size"""
    cv = CURVES[name]
    n = 96
    assert int(os.environ.get("ECAMD_COMB_MIN_BATCH", "4096")) <= n and "ECAMD_NO_COMB" not in os.environ
    h, o = handles(name), oracle(cv)
    ql = U.qlen(cv)
    rs = U.Stream("comb/" + name)
    ks = U.crafted_scalars(cv, ql) + [rs.below(1 << (8 * ql)) for _ in range(n)]
    sc = b"".join(k.to_bytes(ql, "big") for k in ks[:n])
    exp = o.scalar_mult(sc)
    assert h.scalar_mult(sc) == exp          # builds the comb where there is one
    assert h.scalar_mult(sc) == exp          # and answers from it
    G = (cv["gx"], cv["gy"])
    for i in (3, 20, n - 1):
        assert exp[0][2 * U.clen(cv) * i:2 * U.clen(cv) * (i + 1)] == U.pt_bytes(U.mul(ks[i], G, cv), cv)


@pytest.mark.parametrize("name", NAMES)
def test_ecdsa_sign_and_verify(handles, name):
    cv = CURVES[name]
    h, o = handles(name), oracle(cv)
    ql, hl = U.qlen(cv), U.hash_of(cv)().digest_size
    privs, nonces, _, _, digests = U.sign_batch(cv)
    def mask(res):       # the signature bytes of a refused item are not specified
        return b"".join(res[0][2 * ql * i:2 * ql * (i + 1)] if res[1][i] == 0 else bytes(2 * ql) for i in range(len(res[1]))), res[1]
    masked, st = mask(h.ecdsa_sign(privs, nonces, digests, hl))
    assert (masked, st) == mask(o.ecdsa_sign(privs, nonces, digests, hl))
    if cv["ref"] is not None:
        assert U.pack(U.ref_items(cv, "sign"), st, masked) == cv["ref"]["sign"]
    idx = [0, 12, 13, 14, 15, 16, 18]
    items = [(int.from_bytes(privs[ql * i:ql * (i + 1)], "big"), int.from_bytes(nonces[ql * i:ql * (i + 1)], "big"),
              digests[hl * i:hl * (i + 1)]) for i in idx]
    assert U.py_sign(cv, items) == (b"".join(masked[2 * ql * i:2 * ql * (i + 1)] for i in idx), bytes(st[i] for i in idx))

    pubs, vs, _, _, vd, by_msg = U.verify_batch(cv)
    res = h.ecdsa_verify(pubs, vs, vd, hl)
    assert res == o.ecdsa_verify(pubs, vs, vd, hl)
    tail = 0 if 8 * hl > cv["q"].bit_length() else 1
    assert res[:6] == bytes(6) and res[10] == tail and set(res[6:10] + res[11:]) == {1}
    if cv["ref"] is not None:
        rec = bytes.fromhex(cv["ref"]["verify"])
        assert [rec[i] for i in range(len(res)) if by_msg[i]] == [res[i] for i in range(len(res)) if by_msg[i]]


@pytest.mark.parametrize("name", NAMES)
def test_y_from_x_and_decompression(handles, name):
    cv = CURVES[name]
    h, o = handles(name), oracle(cv)
    xs = U.yfx_batch(cv)
    cl = U.clen(cv)
    n = len(xs) // cl
    got = h.y_from_x(xs)
    assert got == o.y_from_x(xs)
    if cv["ref"] is not None:
        assert U.pack(U.ref_items(cv, "yfx"), got[2], got[0], got[1]) == cv["ref"]["yfx"]
    py = U.py_y_from_x(cv, xs)
    for i, roots in enumerate(py):
        assert (got[2][i] == 0) == (roots is not None), i
        if roots is not None:
            assert {int.from_bytes(got[0][cl * i:cl * (i + 1)], "big"), int.from_bytes(got[1][cl * i:cl * (i + 1)], "big")} == roots, i
    # decompression (SEC 1: 02 / 03, then x): the root of the parity asked for (y = 0 has one parity only: left out)
    ask = [(i, par) for i in range(n) for par in (0, 1) if py[i] != {0}]
    comp = b"".join(bytes([2 + par]) + xs[cl * i:cl * (i + 1)] for i, par in ask)
    out, dst = h.decompress(comp)
    for j, (i, par) in enumerate(ask):
        if py[i] is None:
            assert dst[j] == 1, (i, par)
        else:
            y = [v for v in py[i] if v % 2 == par][0]
            assert dst[j] == 0 and out[2 * cl * j:2 * cl * (j + 1)] == xs[cl * i:cl * (i + 1)] + y.to_bytes(cl, "big"), (i, par)


@pytest.mark.parametrize("name", ["U200B", "U544A"])
def test_secret_scalar_mode_gives_the_same_bytes(gpu_ctx, handles, name):
    """one 7-word and one 17-word curve: masked table look-ups change nothing in the answers"""
    cv = CURVES[name]
    h, o = handles(name), oracle(cv)
    hl = U.hash_of(cv)().digest_size
    privs, nonces, _, _, digests = U.sign_batch(cv)
    batches = [b for b in U.smul_batches(cv) if b[0] in ("fixed/q", "var/q", "var/long")]
    gpu_ctx.set_secret_scalars(True)
    try:
        secret = [h.scalar_mult(sc, pts, slen=slen) for _, slen, sc, pts in batches]
        signed = h.ecdsa_sign(privs, nonces, digests, hl)
    finally:
        gpu_ctx.set_secret_scalars(False)
    assert secret == [o.scalar_mult(sc, pts, slen=slen) for _, slen, sc, pts in batches]
    assert secret == [h.scalar_mult(sc, pts, slen=slen) for _, slen, sc, pts in batches]
    plain = h.ecdsa_sign(privs, nonces, digests, hl)
    assert signed[1] == plain[1] == o.ecdsa_sign(privs, nonces, digests, hl)[1]
    ql = U.qlen(cv)
    for i in range(len(plain[1])):
        if plain[1][i] == 0:
            assert signed[0][2 * ql * i:2 * ql * (i + 1)] == plain[0][2 * ql * i:2 * ql * (i + 1)], i
    assert signed[0][:2 * ql * 16] == o.ecdsa_sign(privs, nonces, digests, hl)[0][:2 * ql * 16]
