"""The device shims of the radix-2^29 units (tests/u29g_device_shim.hip, tests/u29_device_shim.hip) cross-compile for gfx950
with the product's flags, export every entry point the GPU tests call, and were built on the asm branches of the headers and as
the flavour they are meant to be.  No GPU needed: a header change that breaks the device build of a unit shows here."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import u29_device as D  # noqa: E402

TAGS = list(D.units()) + ["p256"]


@pytest.fixture(scope="module")
def paths():
    return D.build()


def test_the_nine_objects_follow_the_product_build():
    from libecc_amd import build as B
    u = D.units()
    assert list(u) == ["dense", "521m", "255c", "256k", "448g", "384n", "224s", "192s"] and u["dense"] == (B.G29_SIZES, [])
    # every flavoured job of the product has its object, with the product's -D flags but for the kernel file's own
    flav = [(obj, extra) for src, obj, extra in B._jobs() if src == "ecamd_g29_kernel.hip" and any(
        not f.startswith(D.KERNEL_ONLY) for f in extra) and "-DG29_DISPATCH" not in extra]
    assert len(flav) == len(u) - 1
    for obj, extra in flav:
        sizes, flags = u[obj[len("ecamd_g29_"):-2]]
        assert [f"-DG29_PB={sizes[0]}"] + flags[:-1] == [f for f in extra if not f.startswith("-DG29_WAVES=")]
        assert flags[-1] == f"-DSHIM_ONLY_{sizes[0]}"
    assert "-DU29_ASM_MAD" in B.FLAGS and "--offload-arch=gfx950" in B.FLAGS


@pytest.mark.parametrize("tag", TAGS)
def test_object_exports_and_flags(tag, paths):
    so = paths[tag]
    assert os.path.exists(so)
    exported = {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines() if l.strip()}
    missing = [s for s in D.symbols(tag) if s not in exported]
    assert not missing, missing
    # gd_flags() touches no device: the asm MAD branches, and this object's flavour
    assert C.CDLL(so).gd_flags() == 1 | (D.FLAVOUR_ID[tag] << 8)
    # a gfx950 code object is inside
    assert b"gfx950" in open(so, "rb").read()
