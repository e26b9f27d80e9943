"""The radix-2^29 field and point code of the 18 generic units (ecamd_u29g.h, ecamd_jacg.h, ecamd_rcbg.h) as the DEVICE compiles
it: tests/u29g_device_shim.hip built with the product's flags (-DU29_ASM_MAD: the v_mad_u64_u32 chains of ecamd_madchain.h, the
fold MADs with scalar operands, the signed chains of the sparse units -- branches the g++ build of tests/test_u29g_host.py never
takes), on the vectors of tests/u29g_vectors.py: operands at the edges of their bound classes, lazy limbs, canonicalisation
around 2^|p|, exceptional pairs.  Per unit and operation all records go out in one launch, the extreme ones on lane 0, lane 63,
the first lane of the second wave and in the last, partial wave.  Three exact oracles:
  (a) the residues and flags of Python integers, (b) the bound-class assertions of the host test on the device's limbs -- both by
  replaying the vector generators, assertions included, on the device's outputs;
  (c) limb-for-limb equality with the g++ build of the same entry point on the same operands."""
import os
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import u29_device as D  # noqa: E402
import u29g_vectors as V  # noqa: E402

pytestmark = pytest.mark.gpu
FLAGGED = ("add", "rcb", "liftx")   # the operations that return a flag word


@pytest.fixture(scope="module")
def dev_paths():
    """the device objects: built beforehand as a rule; built here when missing or stale.  A failure to build fails the tests."""
    return D.build()


def _launch(dev, f, op, arg, members):
    """members: [(rec, host out, host r)] of one (field, operation, switch).  One launch; oracle (c) on every lane.  Returns the
    device's (out, r) per member."""
    lanes = D.place([rec.edge for rec, _, _ in members])
    assert len(lanes) > 64 and len(lanes) % 64 != 0
    outs, flags = D.run_g(dev, f, op, arg, [members[i][0].ins for i in lanes])
    got = {}
    for lane, i in enumerate(lanes):
        rec, hout, hr = members[i]
        assert outs[lane] == hout, (op, arg, "lane", lane, "record", i, "device", outs[lane], "host", hout)
        if op in FLAGGED:
            assert flags[lane] == hr, (op, arg, "lane", lane, "record", i, flags[lane], hr)
        got[i] = (outs[lane], flags[lane] if op in FLAGGED else 0)
    return [got[i] for i in range(len(members))]


@pytest.mark.parametrize("name,tag,curve,flavour", V.UNITS, ids=[u[0] for u in V.UNITS])
def test_unit_on_the_device(name, tag, curve, flavour, dev_paths):
    import ctypes as C
    t0 = time.time()
    assert V.HOST_FLAGS[tag] == D.units()[tag][1]           # both builds see the same flavour flags
    host = V.host_lib(V.HOST_NAME[tag], V.HOST_FLAGS[tag])
    dev = C.CDLL(dev_paths[tag])
    # the asm branches, and this flavour: a build that fell back to the portable branches cannot pass
    assert dev.gd_flags() == 1 | (D.FLAVOUR_ID[tag] << 8)
    f, gens = V.generators(host, tag, curve, flavour)
    hi, di = (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
    getattr(host, f"g_info_{f.pb}")(hi)
    getattr(dev, f"gd_info_{f.pb}")(di)
    assert list(hi) == list(di)
    ht, dt = (C.c_uint32 * 3)(), (C.c_uint32 * 3)()
    getattr(host, f"g_infot_{f.pb}")(ht)
    getattr(dev, f"gd_infot_{f.pb}")(dt)
    assert list(ht)[:1 if not ht[0] else 3] == list(dt)[:1 if not ht[0] else 3]
    # the records, through the g++ build (which is held to the same assertions)
    done = {n: V.drive(g()) for n, g in gens}
    counts = V.check_counts(f, tag, flavour, done)
    if not ht[0]:
        assert getattr(dev, f"gd_madd_{f.pb}")(None, None, None, None, 0) == -1 and "madd" not in counts and "dblt" not in counts
    assert ("rcb" in counts) == ("mulword" in counts) == (tag in V.MUL_WORD)
    # one launch per (curve image, operation, switch)
    groups = {}
    for n, d in done.items():
        for j, (rec, out, r) in enumerate(d):
            groups.setdefault((id(rec.f), rec.op, rec.arg), []).append((n, j))
    dev_done = {n: [None] * len(d) for n, d in done.items()}
    t1 = time.time()
    for (_, op, arg), where in groups.items():
        members = [done[n][j] for n, j in where]
        res = _launch(dev, members[0][0].f, op, arg, members)
        for (n, j), (out, r) in zip(where, res):
            dev_done[n][j] = (done[n][j][0], out, r)
    # oracles (a) and (b): the generators' own assertions on the device's outputs
    for n, g in gens:
        V.replay(g(), dev_done[n])
    # the multiplication at one lane, one short of a wave, a full wave, one over
    muls = [m for m in done["field"] if m[0].op == "mul" and m[0].arg == 0]
    for n in (1, 63, 64, 65):
        pick = [muls[i % len(muls)] for i in range(n)]      # the two extreme pairs first (and again on lanes 60, 61)
        outs, _ = D.run_g(dev, f, "mul", 0, [m[0].ins for m in pick])
        for i in range(n):
            assert outs[i] == pick[i][1], ("mul", "n", n, "lane", i)
            lx, ly = pick[i][0].ins
            assert f.val(outs[i]) % f.p == f.val(lx) * f.val(ly) * f.Rinv % f.p
    t2 = time.time()
    print("\n%s (%s, %s): %.2f s in all, %.2f s of it launches, comparisons and replay; records per operation %s"
          % (name, tag, curve, t2 - t0, t2 - t1, dict(sorted(counts.items()))))
