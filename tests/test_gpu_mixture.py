"""vampomi_denoise element by element (denoise_kernel, g1_g1d in
vec.hip), where the norm-relative checks of the runs see nothing: small
elements (spike-dominated markers, x1 ~ 1e-6 |r1|), gam1 from the run's first
iterations (1e-6, where g1d cancels ~1e7-fold) to the |sigma| < 1e-10
shortcut, r1 = +-0 and |r1| tens of standard deviations out, mixtures of 2 to
64 components, and the fixed-order sum of x1d at sizes around a wave, a
block, red_blocks' 512 and beyond kRedBlocks * 512 (further grid-stride
trips).

Two references per element (tests/_mix.py; tests/test_mixture_refs.py checks
them on the CPU): the oracle's g1 / g1d, the same operations with glibc's exp,
sqrt and pow, and the spike-and-slab posterior in mpmath at 50 digits.

Bar, per (L, gam1) group: the device's largest |g - ref| / |r| is at most 4x
the oracle's largest on the same inputs, or 8 * 2^-53 if that is larger; the
same for its largest |gd - ref|.  (A 1-2 ulp difference in exp enters each of
the L terms the way the oracle's own rounding does.)  The relative error of g
itself reaches 1e-8 where the spike dominates, in the reference too (the
formula's cancellation y + sigma pkd / pk): never the bar."""
import math

import numpy as np
import pytest

import _mix

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")


def _hold_to_oracle(tag, r1, x1, x1d, ref, oracle_errs):
    eg, ed = _mix.denoise_errs(r1, x1, x1d, ref)
    og, od = oracle_errs
    print(f"{tag}: max|g-ref|/|r| gpu {eg:.3e} oracle {og:.3e}; max|gd-ref| gpu {ed:.3e} oracle {od:.3e}")
    _mix.record("denoise", tag=tag, gpu_g=eg, oracle_g=og, gpu_gd=ed, oracle_gd=od)
    assert eg <= max(4 * og, _mix.DENOISE_FLOOR), (tag, eg, og)
    assert ed <= max(4 * od, _mix.DENOISE_FLOOR), (tag, ed, od)


@pytest.mark.parametrize("L", _mix.DENOISE_LS)
def test_denoise_elementwise(L):
    with va.Data(_mix.N_SMALL, _mix.DENOISE_M) as d:
        for gam1 in _mix.DENOISE_GAM1:
            grp = _mix.denoise_group(L, gam1)
            r1 = grp["r1"]
            x1, x1d, sd = d.denoise(r1, gam1, grp["probs"], grp["vars"])
            assert np.all(np.isfinite(x1)) and np.all(np.isfinite(x1d)) and math.isfinite(sd), gam1
            assert np.all(x1[r1 == 0] == 0), gam1  # +-0: every term of pkd carries the factor y
            if gam1 >= 1e10:  # |sigma| < 1e-10 (src/vamp.cpp:444, 467)
                assert np.array_equal(x1, r1) and np.all(x1d == 1.0), gam1
            _hold_to_oracle(f"L={L} gam1={gam1:g}", r1, x1, x1d, grp["ref"], grp["oracle_errs"])
            assert abs(sd - math.fsum(x1d)) <= 1e-12 * math.fsum(np.abs(x1d)), gam1


@pytest.mark.parametrize("M", _mix.RED_MS)
def test_denoise_reduction_sizes(M):
    probs, vars_s = _mix.denoise_mix(_mix.RED_L)
    r1 = _mix.red_r1(M)
    with va.Data(_mix.N_SMALL, M) as d:
        x1, x1d, sd = d.denoise(r1, _mix.RED_GAM1, probs, vars_s)
        again = d.denoise(r1, _mix.RED_GAM1, probs, vars_s)
    assert np.array_equal(x1, again[0]) and np.array_equal(x1d, again[1]) and sd == again[2]
    assert np.all(np.isfinite(x1)) and np.all(np.isfinite(x1d))
    tot = math.fsum(x1d)
    assert abs(sd - tot) <= 1e-12 * abs(tot), (sd, tot)
    pick = _mix.red_sample(M)
    rs = r1[pick]
    ref = _mix.denoise_ref(rs, _mix.RED_GAM1, probs, vars_s)
    go, gdo = _mix.oracle_denoise(rs, _mix.RED_GAM1, probs, vars_s)
    _hold_to_oracle(f"M={M} L={_mix.RED_L} gam1={_mix.RED_GAM1:g}", rs, x1[pick], x1d[pick], ref,
                    _mix.denoise_errs(rs, go, gdo, ref))
