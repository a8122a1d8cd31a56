"""Missing methylation values (NaN): planted inputs and the fill restated in
numpy, shared by tests/test_meth_na.py and tests/test_gpu_meth_na.py.  Nothing
here touches the engine.

The rule (include/vampomi.h): under the policy "mean" a missing
entry of a marker is replaced by s / n_obs over the marker's observed entries;
a marker with no observed entry, or with (double)n_missing > f * (double)n, is
stored as zeros.  The engine sums in a fixed order of its own, so the reference
here is the exact mean (math.fsum) with the first-order bound of ANY summation
order around it:

    gamma = (n_obs + 1) * 2^-53 * mean|x_obs|

((n_obs - 1) u sum|x| / n_obs for the sum, u |m| for the division and u |m| for
fsum's own rounding, u = 2^-53, |m| <= mean|x|.)
"""
from __future__ import annotations

import math

import numpy as np

# NaNs of every kind: quiet, negative, payload-carrying, signalling
NAN64 = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000ABCDEF, 0xFFFFFFFFFFFFFFFF,
                  0x7FF0000000000001, 0xFFF4000000000000], dtype=np.uint64)
NAN32 = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFFFFFFF, 0x7F800001, 0xFFA00000], dtype=np.uint32)
assert np.all(np.isnan(np.frombuffer(NAN64.tobytes(), dtype=np.float64)))
assert np.all(np.isnan(np.frombuffer(NAN32.tobytes(), dtype=np.float32)))

PATTERNS = ("none", "row0", "last", "runs", "alternate", "all_but_one", "all", "payload")


def pattern_mask(name: str, N: int, rng) -> np.ndarray:
    """The missing rows of one marker.  N >= 301."""
    m = np.zeros(N, dtype=bool)
    if name == "row0":
        m[0] = True
    elif name == "last":
        m[N - 1] = True
    elif name == "ends":
        m[[0, N - 1]] = True
    elif name == "runs":  # 64 and 65 consecutive rows: a whole wave's lanes, and one more
        m[10:74] = True
        m[100:165] = True
    elif name == "alternate":
        m[::2] = True
    elif name == "all_but_one":
        m[:] = True
        m[N // 2] = False
    elif name == "all":
        m[:] = True
    elif name == "payload":
        m[[1, 5, 63, 64, N - 2]] = True
    elif name == "random":  # 0.5 %
        m[rng.choice(N, max(1, int(round(0.005 * N))), replace=False)] = True
    elif name != "none":
        raise ValueError(name)
    return m


def plant_mask(N: int, M: int, patterns=None, seed: int = 77) -> np.ndarray:
    """(M, N) bool: marker i gets patterns[i] (default: PATTERNS in order), the
    markers past the list 0.5 % at random from the fixed seed."""
    rng = np.random.default_rng(seed)
    patterns = PATTERNS if patterns is None else patterns
    return np.stack([pattern_mask(patterns[i] if i < len(patterns) else "random", N, rng) for i in range(M)])


def with_nans(X: np.ndarray, mask: np.ndarray, dtype) -> np.ndarray:
    """X as dtype (float64 / float32) with a NaN at every masked entry: bit
    patterns of every kind in turn, written through an integer view."""
    Xin = np.ascontiguousarray(X, dtype=dtype).copy()
    bits, pats = (np.uint64, NAN64) if Xin.dtype == np.float64 else (np.uint32, NAN32)
    Xin.view(bits)[mask] = np.resize(pats, int(mask.sum()))
    assert np.array_equal(np.isnan(Xin), mask)
    return Xin


def conv(v, storage: str):
    """What the ingest stores for the value(s) v, as doubles.  u16: the grid's
    rule for v in [0, 1]; the bounds m -+ gamma of a mean of values in [0, 1]
    may leave it by gamma and are taken back in."""
    v = np.asarray(v, dtype=np.float64)
    if storage == "f64":
        return v
    if storage == "f32":
        return v.astype(np.float32).astype(np.float64)
    if storage == "u16":
        return np.minimum(65535, np.rint(np.clip(v, 0.0, 1.0) * 65536)) / 65536
    raise ValueError(storage)


def fill_reference(Xin: np.ndarray, max_frac: float = 1.0) -> dict:
    """Per marker of Xin (M, n; the kept rows only): counts (int64), masked
    (bool), mean (the exact mean of the observed entries, correctly rounded;
    0 where there is none) and gamma."""
    M, n = Xin.shape
    counts = np.zeros(M, dtype=np.int64)
    masked = np.zeros(M, dtype=bool)
    mean = np.zeros(M)
    gamma = np.zeros(M)
    for i in range(M):
        with np.errstate(invalid="ignore"):  # (widening a signalling NaN raises the flag)
            x = Xin[i].astype(np.float64)  # (floats widen exactly)
        miss = np.isnan(x)
        counts[i] = int(miss.sum())
        n_obs = n - int(counts[i])
        masked[i] = n_obs == 0 or float(counts[i]) > max_frac * float(n)
        if n_obs:
            obs = x[~miss]
            mean[i] = math.fsum(obs) / n_obs
            gamma[i] = (n_obs + 1) * 2.0 ** -53 * (math.fsum(np.abs(obs)) / n_obs)
    return {"counts": counts, "masked": masked, "mean": mean, "gamma": gamma,
            "stats": {"missing": int(counts.sum()), "markers_with_missing": int(np.count_nonzero(counts)),
                      "markers_masked": int(np.count_nonzero(masked))}}


def fill_bounds(ref: dict, storage: str):
    """(lo, hi) per marker: the stored fill lies in [conv(m - gamma), conv(m + gamma)]."""
    return conv(ref["mean"] - ref["gamma"], storage), conv(ref["mean"] + ref["gamma"], storage)


def check_filled(stored: np.ndarray, plain: np.ndarray, Xin: np.ndarray, storage: str, max_frac: float = 1.0) -> dict:
    """stored: the read-back (M, n) of a "mean" context loaded with Xin; plain:
    that of a plain context of the same storage loaded with Xin's NaNs replaced
    by any in-range value.  Asserts the read-back rule and returns the reference."""
    ref = fill_reference(Xin, max_frac)
    miss = np.isnan(Xin)
    lo, hi = fill_bounds(ref, storage)
    for i in range(Xin.shape[0]):
        if ref["masked"][i]:
            assert not stored[i].any(), f"marker {i}: a masked marker is stored as zeros"
            continue
        assert np.array_equal(stored[i][~miss[i]], plain[i][~miss[i]]), f"marker {i}: observed entries"
        if ref["counts"][i]:
            f = stored[i][miss[i]]
            assert np.all(f == f[0]), f"marker {i}: one fill per marker"
            assert lo[i] <= f[0] <= hi[i], (i, lo[i], f[0], hi[i], ref["mean"][i], ref["gamma"][i])
    return ref
