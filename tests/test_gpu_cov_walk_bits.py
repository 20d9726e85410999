"""ksx_kernel and believer_kernel walk the observations with one text (csrc/ksx_walk.h), kg_kernel with a copy of it; this pins the
bits of what the three make, case by case, against tests/golden/cov_walk_bits.json (tools/cov_walk_bits.py states the cases and what each one hashes).
A mismatch fails -- it never skips."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("cov_walk_bits", os.path.join(ROOT, "tools", "cov_walk_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wctx():
    import bot7_amd
    c = bot7_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    return bits.recorded()["sha256"]


def test_every_case_is_recorded(want):
    assert sorted(want) == sorted(bits.case_ids())


@pytest.mark.parametrize("cid", bits.case_ids())
def test_cov_walk_bits(wctx, want, cid):
    got = bits.case_hash(wctx, cid)
    print(cid, got)
    assert got == want[cid], "%s: the bits moved (%s, recorded %s).  %s" % (cid, got, want[cid], bits.REGEN)
