"""The association tests' bits against a record (tests/golden/assoc_bits_pin.json).

The workgroup kernel of one phenotype and the kernels of several share one
body, so "a block equals the single call" (tests/test_gpu_assoc_multi.py)
compares that body with itself at eight waves.  This test holds what both
return to SHA-256 digests recorded from the library as it was before the two
bodies became one: assoc_loo at the default variant and at the wave-per-marker
variant 0, assoc_loo_multi at T = 2 ... 5 and assoc_loco with and without an
estimate, on the small shapes and storages of tools/assoc_pin.py, which made
the record and makes the digests here.  The test never writes the record."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import assoc_pin  # noqa: E402


def test_association_bits_equal_the_record():
    ref = assoc_pin.recorded()
    # 8 cases x (2 variants + 4 widths + 2 LOCO calls) x (p-values, statistics)
    assert len(ref) == len(assoc_pin.CASES) * 8 * 2 == 128
    got = assoc_pin.digests()
    assert sorted(got) == sorted(ref)
    bad = sorted(k for k in ref if got[k] != ref[k])
    assert not bad, bad
