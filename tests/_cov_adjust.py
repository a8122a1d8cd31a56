"""Shared pieces of the covariate-adjustment tests (tests/test_cov_adjust.py,
tests/test_gpu_cov_adjust.py): covariate tables with planted degenerate
columns, the numpy reference of the adjustment, and the files of a run."""
import numpy as np


def covariates(n: int, C: int, seed: int = 3):
    """(Z, dropped): an (n, C) table of raw covariates, uniform in (-1, 1) and
    well conditioned apart from what is planted: from C = 5 on column 1 is a
    constant, column 3 a copy of column 0 and column 4 a linear combination of
    columns 0, 2 and the intercept; from C = 64 on column 40 is all zero."""
    rng = np.random.default_rng(seed + 1000 * C + n)
    Z = rng.uniform(-1.0, 1.0, (n, C))
    dropped = np.zeros(C, dtype=bool)
    if C >= 5:
        Z[:, 1] = 2.5
        Z[:, 3] = Z[:, 0]
        Z[:, 4] = 0.5 * Z[:, 0] - 2.0 * Z[:, 2] + 1.0
        dropped[[1, 3, 4]] = True
    if C >= 64:
        Z[:, 40] = 0.0
        dropped[40] = True
    return Z, dropped


def design(Z: np.ndarray, dropped=None) -> np.ndarray:
    """[1, Z] without the dropped columns."""
    Z = np.asarray(Z, dtype=np.float64)
    keep = np.ones(Z.shape[1], dtype=bool) if dropped is None else ~np.asarray(dropped, dtype=bool)
    return np.hstack([np.ones((Z.shape[0], 1)), Z[:, keep]])


def residual(Z1: np.ndarray, V: np.ndarray) -> np.ndarray:
    """V - Z1 lstsq(Z1, V) for the columns of V (n, k) (or a vector)."""
    return V - Z1 @ np.linalg.lstsq(Z1, V, rcond=None)[0]


def plant(X: np.ndarray, z: np.ndarray, kinds):
    """X (M, N) with planted markers, in place; z: the first covariate.  kinds:
    names in marker order from marker 0; "pair" takes two markers (a copy of
    the first in the second).  Returns {kind: marker}."""
    at, i = {}, 0
    for k in kinds:
        at[k] = i
        if k == "const":
            X[i] = 0.5
        elif k == "zero":
            X[i] = 0.0
        elif k == "cov":
            X[i] = z
        elif k == "affine":
            X[i] = 0.3 * z + 0.2
        elif k == "pair":
            X[i + 1] = X[i]
            i += 1
        else:
            raise ValueError(k)
        i += 1
    return at


def write_cov(path, Z: np.ndarray):
    """The covariate file of Z (n, C): a header, then FID IID and C numbers that
    parse back to the same doubles."""
    with open(path, "w") as f:
        f.write("FID IID " + " ".join("c%d" % j for j in range(Z.shape[1])) + "\n")
        for i, row in enumerate(Z):
            f.write("f%d i%d " % (i, i) + " ".join(repr(float(v)) for v in row) + "\n")


def write_phen(path, y: np.ndarray):
    with open(path, "w") as f:
        for i, v in enumerate(y):
            f.write("f%d i%d %s\n" % (i, i, repr(float(v))))
