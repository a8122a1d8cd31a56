"""vampomi_amd — MI355X-native gVAMPomi VAMP engine (host-side mirror).

The compute lives in libvampomi.so (HIP kernels for gfx950 + RCCL, C ABI in
include/vampomi.h).  This module mirrors the reference's operator interface
so code written against it reads like the reference:

* :class:`Data` — the reference's ``class data`` (src/data.hpp:11-92):
  phenotype + marker-major fp64 shard, ``Ax`` / ``ATx`` / ``get_mave`` /
  ``get_msig`` / ``get_phen``;
* :class:`Vamp` — the reference's ``class vamp`` (src/vamp.hpp:7-151):
  ``infere`` runs ``infere_linear`` on the device, plus the step-wise API used
  by bench.py;
* :func:`divide_work` — src/utilities.cpp:207-239.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from ._lib import (CLI_PATH, GEN_GAUSS, GEN_METH, LIB_PATH, MAX_L, MEM_DEVICE, MEM_HOST, NA_FATAL, NA_MEAN, NA_PASS,
                   STORE_F32, STORE_F64, STORE_U16, UNIQUE_ID_BYTES, Params, Result, ShardDesc, Stats, VampomiError,
                   check, load)

__all__ = ["Data", "Vamp", "VampOptions", "divide_work", "comm_unique_id", "phen_rows", "phen_rows_common", "read_labels", "adjust_basis", "VampomiError", "LIB_PATH", "CLI_PATH",
           "GEN_GAUSS", "GEN_METH", "STORE_F64", "STORE_F32", "STORE_U16", "load"]

_STORAGE = {"f64": STORE_F64, "f32": STORE_F32, "u16": STORE_U16}
_METH_NA = {"pass": NA_PASS, "fatal": NA_FATAL, "mean": NA_MEAN}


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def divide_work(Mt: int, nranks: int, rank: int):
    """(M, S, Mm) of ``rank`` — src/utilities.cpp:207-239."""
    M, S, Mm = C.c_int64(), C.c_int64(), C.c_int64()
    load().vampomi_divide_work(Mt, nranks, rank, C.byref(M), C.byref(S), C.byref(Mm))
    return M.value, S.value, Mm.value


def comm_unique_id() -> bytes:
    """RCCL unique id (rank 0 creates it, the caller broadcasts it)."""
    buf = (C.c_ubyte * UNIQUE_ID_BYTES)()
    check(load().vampomi_comm_unique_id(buf))
    return bytes(buf)


def phen_rows(path: str, keep_file: Optional[str] = None, drop_na: bool = False):
    """(rows, N_file): the ascending rows of the PLINK phenotype file ``path``
    that an analysis keeps, and the file's row count (vampomi_phen_rows; no
    device needed).  ``keep_file``: PLINK ``--keep`` style, FID and IID per
    line; ``drop_na``: rows whose value is ``NA`` are dropped too (else an
    ``NA`` in a kept row raises status 5).  Pass them as ``Data(N_file, Mt,
    rows=rows)``."""
    lib = load()
    keep = None if keep_file is None else keep_file.encode()
    nf, n = C.c_int64(), C.c_int64()
    check(lib.vampomi_phen_rows(path.encode(), keep, 1 if drop_na else 0, None, 0, C.byref(nf), C.byref(n)))
    rows = np.zeros(max(n.value, 1), dtype=np.int64)
    check(lib.vampomi_phen_rows(path.encode(), keep, 1 if drop_na else 0, _dp(rows), n.value, C.byref(nf),
                                C.byref(n)))
    return rows[: n.value], nf.value


def phen_rows_common(paths, keep_file: Optional[str] = None, drop_na: bool = False):
    """(rows, N_file, na_per_file): the ascending rows that an analysis of all
    the PLINK phenotype files ``paths`` keeps (vampomi_phen_rows_common; no
    device needed).  The files must list the same individuals in the same
    order (else status 1, the message naming the first differing file and
    row).  ``keep_file`` as :func:`phen_rows`'s; with ``drop_na`` a row is kept
    iff it is kept and not ``NA`` in every file, else an ``NA`` in a kept row
    of any file raises status 5 naming the file.  ``na_per_file``: the ``NA``
    count of each file among the rows the keep file leaves."""
    lib = load()
    paths = [str(p) for p in paths]
    arr = (C.c_char_p * max(len(paths), 1))(*[p.encode() for p in paths])
    keep = None if keep_file is None else str(keep_file).encode()
    nf, n = C.c_int64(), C.c_int64()
    na = np.zeros(max(len(paths), 1), dtype=np.int64)
    check(lib.vampomi_phen_rows_common(arr, len(paths), keep, 1 if drop_na else 0, None, 0, C.byref(nf), C.byref(n),
                                       _dp(na)))
    rows = np.zeros(max(n.value, 1), dtype=np.int64)
    check(lib.vampomi_phen_rows_common(arr, len(paths), keep, 1 if drop_na else 0, _dp(rows), n.value, C.byref(nf),
                                       C.byref(n), _dp(na)))
    return rows[: n.value], nf.value, na[: len(paths)]


def read_labels(path: str, Mt: int):
    """(labels, names): the --loco-file ``path`` (vampomi_read_labels; no
    device needed).  The file holds exactly ``Mt`` whitespace-separated tokens,
    one per marker in file order; ``labels`` (int32, Mt) numbers them by first
    appearance and ``names`` lists the distinct tokens in that order.  Another
    token count or more than 64 distinct tokens raises status 1."""
    lib = load()
    lab = np.zeros(max(int(Mt), 1), dtype=np.int32)
    G = C.c_int()
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        st = lib.vampomi_read_labels(str(path).encode(), int(Mt), _dp(lab), C.byref(G), buf, cap)
        if st == 1 and b"names_cap" in lib.vampomi_last_error() and cap < (1 << 28):
            cap *= 16
            continue
        check(st)
        break
    names = buf.value.decode().split("\n")[: G.value]
    return lab[: int(Mt)], names


def adjust_basis(Z: np.ndarray):
    """(Q, dropped): the orthonormal basis of span{1, Z} that a covariate
    adjustment projects out (vampomi_adjust_basis; no device needed).  ``Z``:
    (n, C) raw covariates, C >= 0.  ``Q``: (n, R), its first column the
    intercept's 1/sqrt(n); ``dropped``: C booleans, the constant or dependent
    columns of ``Z``."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim != 2:
        raise ValueError("Z must be (n, C)")
    n, nc = Z.shape
    Zc = np.ascontiguousarray(Z.T)  # covariate-major
    Q = np.zeros((nc + 1, max(n, 1)))
    dropped = np.zeros(max(nc, 1), dtype=np.int32)
    R = C.c_int()
    check(load().vampomi_adjust_basis(_dp(Zc), n, nc, n, _dp(Q), C.byref(R), _dp(dropped)))
    return np.ascontiguousarray(Q[: R.value].T), dropped[:nc].astype(bool)


class Data:
    """Device-resident marker shard + phenotype (reference ``class data``).

    ``Data(N, Mt, rank, nranks)`` owns markers ``[S, S+M)`` of ``Mt``
    (divide_work).  Load the shard with :meth:`read_methylation_data` (file),
    :meth:`load_meth` (numpy, shape (M, N) marker-major) or :meth:`generate`
    (on-device synthetic); the phenotype with :meth:`read_phen` or
    :meth:`set_phen`.  Marker statistics are computed at load
    (compute_markers_statistics, src/data.cpp:233-283).

    ``storage``: how the shard is held on the device, ``"f64"``, ``"f32"`` or
    ``"u16"`` (None: the library's default, ``"f64"`` unless ``VAMPOMI_STORAGE``
    says otherwise).  With ``"f32"`` the matrix takes half the memory and every
    pass reads half the bytes; fp64 input is rounded to nearest even at ingest.
    With ``"u16"`` it takes a quarter: a value in [0, 1] is stored as the
    ``uint16`` ``k = min(65535, rint(x * 65536))`` meaning ``k / 65536`` (at most
    7.7e-6 off); NaN, infinities and values outside [0, 1] fail the load with
    ``VampomiError`` (status 9, ``ERR_RANGE``; the message names the first such
    entry), and :meth:`quant_stats` tells what the quantisation did.  All
    arithmetic stays fp64.  The ``storage`` attribute tells which is in use.

    ``rows``: a row subset (:func:`phen_rows`).  ``N`` is then the row count of
    the FILES, the context is opened with ``len(rows)`` samples, ``d.N ==
    len(rows)``, and ``d.N_file`` and ``d.rows`` tell the rest.  The loads
    (:meth:`read_methylation_data`, :meth:`load_meth` with an ``(M, N_file)``
    array, :meth:`read_phen`, :meth:`read_covariates`) take the full files and
    keep those rows; the context then holds, bit for bit, what a plain one
    holds after loading files with the other rows removed.  :meth:`set_phen`
    and :meth:`set_covariates` keep taking ``d.N`` rows.

    ``meth_na``: what a load does with a missing methylation value, a NaN of
    fp64 or fp32 input (uint16 input has none).  ``"pass"`` (the default):
    nothing, as ever.  ``"fatal"``: the load raises ``VampomiError`` (status 10,
    ``ERR_NAN_METH``; the message gives their number and the first marker and
    row).  ``"mean"``: each is replaced by the mean of the marker's observed
    entries among the kept rows, stored as any input value is; a marker with no
    observed entry, or with more than ``max_missing_frac`` of its entries
    missing, is stored as zeros, a constant column that the model sees as
    exactly null.  Everything after the load treats the filled matrix
    (:meth:`get_meth_data`) as the data.  :meth:`missing_stats` and
    :meth:`missing_counts` tell what the last load found.

    ``adjust``: covariates to regress out of the LINEAR model's data at ingest,
    an intercept always with them.  Either a ``(d.N, C)`` array of raw values
    (the kept rows; ``C`` may be 0: the intercept only), or the path of a
    covariate file together with ``adjust_C``, its number of columns (the file
    has ``N_file`` rows, of which a row subset's are taken).  Every load then
    stores each marker's residual on span{1, Z} (after the row gather and the
    ``meth_na`` fill, in fp64, rounded once into ``"f32"``; ``"u16"`` cannot
    hold residuals: status 1), a marker inside that span is stored as zeros
    (absorbed), and :meth:`read_phen` / :meth:`set_phen` project the phenotype
    the same way before they scale it.  :meth:`adjust_info` and
    :meth:`adjust_stats` tell the rest.  :meth:`generate` and the
    ``"bin_class"`` model raise status 6 on such a context.
    """

    def __init__(self, N: int, Mt: int, rank: int = 0, nranks: int = 1, comm_id: Optional[bytes] = None,
                 device: int = -1, alpha_scale: float = 1.0, storage: Optional[str] = None,
                 rows: Optional[Sequence[int]] = None, meth_na: Optional[str] = None, max_missing_frac: float = 1.0,
                 adjust=None, adjust_C: Optional[int] = None):
        if isinstance(adjust, str) != (adjust_C is not None):
            raise ValueError("adjust_C goes with adjust=<path of a covariate file>, and only with it")
        if storage is not None and storage not in _STORAGE:
            raise ValueError(f'storage must be "f64", "f32" or "u16", not {storage!r}')
        if meth_na is not None and meth_na not in _METH_NA:
            raise ValueError(f'meth_na must be "pass", "fatal" or "mean", not {meth_na!r}')
        if max_missing_frac != 1.0 and meth_na != "mean":
            raise ValueError('max_missing_frac needs meth_na="mean"')
        self.N_file, self.rows = N, None
        if rows is not None:
            self.rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
            N = len(self.rows)
        self._lib = load()
        self._idbuf = None
        d = ShardDesc(N=N, Mt=Mt, rank=rank, nranks=nranks, device=device, comm_id=None, alpha_scale=alpha_scale)
        if nranks > 1:
            if comm_id is None or len(comm_id) != UNIQUE_ID_BYTES:
                raise ValueError("nranks > 1 needs the 128-byte communicator id from rank 0")
            self._idbuf = (C.c_ubyte * UNIQUE_ID_BYTES).from_buffer_copy(comm_id)
            d.comm_id = C.cast(self._idbuf, C.c_void_p)
        h = C.c_void_p()
        check(self._lib.vampomi_open(C.byref(d), C.byref(h)))
        self.ctx = h
        self.N, self.Mt, self.rank, self.nranks = N, Mt, rank, nranks
        self.C = 0  # covariates held (set_covariates / read_covariates)
        M, S, ld = C.c_int64(), C.c_int64(), C.c_int64()
        check(self._lib.vampomi_shard_info(self.ctx, C.byref(M), C.byref(S), C.byref(ld)))
        self.M, self.S, self.ld = M.value, S.value, ld.value
        if storage is not None:
            check(self._lib.vampomi_set_storage(self.ctx, _STORAGE[storage]))
        if self.rows is not None:
            check(self._lib.vampomi_set_row_subset(self.ctx, self.N_file, _dp(self.rows), len(self.rows)))
        if meth_na is not None:
            check(self._lib.vampomi_set_meth_na(self.ctx, _METH_NA[meth_na], max_missing_frac))
        if isinstance(adjust, str):
            check(self._lib.vampomi_read_adjust(self.ctx, adjust.encode(), adjust_C))
        elif adjust is not None:
            Z = np.asarray(adjust, dtype=np.float64)
            if Z.ndim != 2 or Z.shape[0] != self.N:
                raise ValueError(f"adjust must be ({self.N}, C), got {Z.shape}")
            Zc = np.ascontiguousarray(Z.T)  # covariate-major
            check(self._lib.vampomi_set_adjust(self.ctx, _dp(Zc) if Z.shape[1] else None, Z.shape[1], self.N))

    def adjust_info(self) -> dict:
        """The adjustment: ``R`` basis vectors (0: none), ``dropped`` (one
        boolean per covariate column: constant or dependent) and ``Q``, (N, R),
        the orthonormal basis, the intercept's column first."""
        R = C.c_int()
        check(self._lib.vampomi_get_adjust(self.ctx, C.byref(R), None, None))
        dropped = np.zeros(65, dtype=np.int32)
        dropped[:] = -1
        Q = np.zeros((max(R.value, 1), self.N))
        check(self._lib.vampomi_get_adjust(self.ctx, None, _dp(dropped), _dp(Q)))
        return {"R": R.value, "dropped": dropped[dropped >= 0].astype(bool),
                "Q": np.ascontiguousarray(Q[: R.value].T)}

    def adjust_stats(self) -> dict:
        """What the last load's adjustment did to this shard: ``absorbed``, the
        markers stored as zeros because nothing of them was left outside the
        covariates' span, and ``flags``, one boolean per local marker."""
        n = C.c_int64()
        flags = np.zeros(max(self.M, 1), dtype=np.uint8)
        check(self._lib.vampomi_get_adjust_stats(self.ctx, C.byref(n), _dp(flags)))
        return {"absorbed": n.value, "flags": flags[: self.M].astype(bool)}

    @property
    def meth_na(self) -> str:
        p, f = C.c_int(), C.c_double()
        check(self._lib.vampomi_get_meth_na(self.ctx, C.byref(p), C.byref(f)))
        return {NA_FATAL: "fatal", NA_MEAN: "mean"}.get(p.value, "pass")

    @property
    def max_missing_frac(self) -> float:
        p, f = C.c_int(), C.c_double()
        check(self._lib.vampomi_get_meth_na(self.ctx, C.byref(p), C.byref(f)))
        return f.value

    def missing_stats(self) -> dict:
        """What the last load found in this shard: ``missing`` entries (NaN, among
        the kept rows), ``markers_with_missing``, and ``markers_masked`` (stored
        as zeros under ``"mean"``).  Zeros under ``"pass"``, which does not look."""
        a, b, m = C.c_int64(), C.c_int64(), C.c_int64()
        check(self._lib.vampomi_get_missing_stats(self.ctx, C.byref(a), C.byref(b), C.byref(m), None))
        return {"missing": a.value, "markers_with_missing": b.value, "markers_masked": m.value}

    def missing_counts(self) -> np.ndarray:
        """The missing entries of each local marker (int64, M; a masked marker's
        true count)."""
        out = np.zeros(max(self.M, 1), dtype=np.int64)
        check(self._lib.vampomi_get_missing_stats(self.ctx, None, None, None, _dp(out)))
        return out[: self.M]

    @property
    def storage(self) -> str:
        s = C.c_int()
        check(self._lib.vampomi_get_storage(self.ctx, C.byref(s)))
        return {STORE_F32: "f32", STORE_U16: "u16"}.get(s.value, "f64")

    def quant_stats(self) -> dict:
        """What the last load of a ``"u16"`` shard did to its input: ``clamped``,
        the entries in [1 - 2**-17, 1] stored as 65535/65536, and
        ``max_abs_err``, the largest |stored - input|.  Zeros for the other
        storages."""
        n, e = C.c_int64(), C.c_double()
        check(self._lib.vampomi_get_quant_stats(self.ctx, C.byref(n), C.byref(e)))
        return {"clamped": n.value, "max_abs_err": e.value}

    # -- lifecycle --
    def close(self):
        if getattr(self, "ctx", None):
            self._lib.vampomi_close(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        check(self._lib.vampomi_sync(self.ctx))

    def barrier(self):
        check(self._lib.vampomi_barrier(self.ctx))

    # -- ingest --
    def read_methylation_data(self, path: str, dtype: str = "f64"):
        """The marker-major file's elements are doubles (``"f64"``), floats
        (``"f32"``) or little-endian ``uint16`` k meaning k / 65536 (``"u16"``);
        any of them loads into any storage."""
        if dtype not in _STORAGE:
            raise ValueError(f'dtype must be "f64", "f32" or "u16", not {dtype!r}')
        load_file = {"f64": self._lib.vampomi_load_meth_file, "f32": self._lib.vampomi_load_meth_file_f32,
                     "u16": self._lib.vampomi_load_meth_file_u16}[dtype]
        check(load_file(self.ctx, path.encode()))

    def load_meth(self, X: np.ndarray):
        """X: (M, N), this shard's markers (marker-major): float64, float32
        (passed as it is, with no upcast copy) or uint16 (k meaning k / 65536),
        for any storage.  With a row subset: (M, N_file)."""
        if getattr(X, "dtype", None) == np.float32:
            X = np.ascontiguousarray(X)
            load_host = self._lib.vampomi_load_meth_host_f32
        elif getattr(X, "dtype", None) == np.uint16:
            X = np.ascontiguousarray(X)
            load_host = self._lib.vampomi_load_meth_host_u16
        else:
            X = np.ascontiguousarray(X, dtype=np.float64)
            load_host = self._lib.vampomi_load_meth_host
        if X.shape != (self.M, self.N_file):
            raise ValueError(f"expected shard shape {(self.M, self.N_file)}, got {X.shape}")
        check(load_host(self.ctx, _dp(X), self.N_file))

    def generate(self, seed: int, kind: int = GEN_GAUSS):
        check(self._lib.vampomi_generate_meth(self.ctx, seed, kind))

    def read_phen(self, path: str, standardize: bool = True):
        check(self._lib.vampomi_read_phen(self.ctx, path.encode(), 1 if standardize else 0))

    def set_phen(self, y: np.ndarray, standardize: bool = True):
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (self.N,):
            raise ValueError("phenotype must have N entries")
        check(self._lib.vampomi_set_phen(self.ctx, _dp(y), 1 if standardize else 0))

    # -- covariates of the probit model (data::read_covariates, src/data.cpp:159-227) --
    def read_covariates(self, path: str, C: int):
        """Header line, then per row two IDs and C numbers; standardised per
        column (population deviation; a constant column becomes zeros)."""
        check(self._lib.vampomi_read_covariates(self.ctx, path.encode(), C))
        self.C = C

    def set_covariates(self, Z: Optional[np.ndarray], standardize: bool = True):
        """Z: (N, C), one row per sample (None or C == 0: no covariates)."""
        if Z is None or np.size(Z) == 0:
            check(self._lib.vampomi_set_covariates(self.ctx, None, 0, self.N, 0))
            self.C = 0
            return
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[0] != self.N:
            raise ValueError("covariates must be an (N, C) array")
        Zt = np.ascontiguousarray(Z.T)  # covariate-major
        check(self._lib.vampomi_set_covariates(self.ctx, _dp(Zt), Z.shape[1], self.N, 1 if standardize else 0))
        self.C = Z.shape[1]

    def get_covariates(self) -> np.ndarray:
        """The stored (standardised) table, (N, C)."""
        C_ = getattr(self, "C", 0)
        out = np.zeros((max(C_, 1), self.N))
        check(self._lib.vampomi_get_covariates(self.ctx, _dp(out)))
        return np.ascontiguousarray(out[:C_].T)

    def cov_eval(self, eta: np.ndarray, gg: Optional[np.ndarray] = None):
        """One evaluation of Newton_method_cov's sums (src/vamp_probit.cpp:536-551):
        (H (C, C), rhs (C), mlogL) at eta with the genetic predictor gg (None: zeros)."""
        C_ = getattr(self, "C", 0)
        eta = np.ascontiguousarray(eta, dtype=np.float64)
        if eta.shape != (C_,):
            raise ValueError("eta must have C entries")
        g = None if gg is None else np.ascontiguousarray(gg, dtype=np.float64)
        H, rhs, ml = np.zeros((max(C_, 1), max(C_, 1))), np.zeros(max(C_, 1)), C.c_double()
        check(self._lib.vampomi_cov_eval(self.ctx, None if g is None else _dp(g), _dp(eta), _dp(H), _dp(rhs),
                                         C.byref(ml), MEM_HOST))
        return H[:C_, :C_], rhs[:C_], ml.value

    def newton_cov(self, gg: Optional[np.ndarray] = None, eta0: Optional[np.ndarray] = None):
        """vamp::Newton_method_cov (:525-617): (eta, outer iterations, backtracks
        per iteration, rel_err per iteration)."""
        C_ = getattr(self, "C", 0)
        g = None if gg is None else np.ascontiguousarray(gg, dtype=np.float64)
        e0 = None if eta0 is None else np.ascontiguousarray(eta0, dtype=np.float64)
        eta = np.zeros(max(C_, 1))
        it = C.c_int()
        bt = np.zeros(501, dtype=np.int32)
        rel = np.zeros(501)
        check(self._lib.vampomi_newton_cov(self.ctx, None if g is None else _dp(g), None if e0 is None else _dp(e0),
                                           _dp(eta), C.byref(it), _dp(bt), _dp(rel), MEM_HOST))
        return eta[:C_], it.value, bt[: it.value].copy(), rel[: it.value].copy()

    def simulate_phen_binary(self, seed: int, lam: float = 0.1, h2: float = 0.8) -> np.ndarray:
        """Liability of simulate_phen thresholded at 0, stored raw (bin_class); returns beta."""
        beta = np.zeros(max(self.M, 1))
        check(self._lib.vampomi_simulate_phen_binary(self.ctx, seed, lam, h2, _dp(beta)))
        return beta[: self.M]

    def simulate_phen(self, seed: int, lam: float = 0.1, h2: float = 0.8) -> np.ndarray:
        beta = np.zeros(max(self.M, 1))
        check(self._lib.vampomi_simulate_phen(self.ctx, seed, lam, h2, _dp(beta)))
        return beta[: self.M]

    # -- accessors (src/data.hpp:48-66) --
    def get_phen(self) -> np.ndarray:
        y = np.zeros(self.N)
        check(self._lib.vampomi_get_phen(self.ctx, _dp(y)))
        return y

    def get_mave(self) -> np.ndarray:
        a = np.zeros(max(self.M, 1))
        check(self._lib.vampomi_get_marker_stats(self.ctx, _dp(a), None))
        return a[: self.M]

    def get_msig(self) -> np.ndarray:
        a = np.zeros(max(self.M, 1))
        check(self._lib.vampomi_get_marker_stats(self.ctx, None, _dp(a)))
        return a[: self.M]

    def get_meth_data(self, i0: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Local markers [i0, i0+count) as a (count, N) array (src/data.hpp:53)."""
        count = self.M - i0 if count is None else count
        out = np.zeros((max(count, 1), self.N))
        check(self._lib.vampomi_read_markers(self.ctx, i0, count, _dp(out)))
        return out[:count]

    # -- operators (src/data.cpp:294-373) --
    def Ax(self, x: np.ndarray) -> np.ndarray:
        """COLLECTIVE: (sum over ranks of (X - mave) * msig * x) / sqrt(N)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros(self.N)
        check(self._lib.vampomi_ax(self.ctx, _dp(x), _dp(out), MEM_HOST))
        return out

    def ATx(self, u: np.ndarray) -> np.ndarray:
        u = np.ascontiguousarray(u, dtype=np.float64)
        out = np.zeros(max(self.M, 1))
        check(self._lib.vampomi_atx(self.ctx, _dp(u), _dp(out), MEM_HOST))
        return out[: self.M]

    def lmmse_mult(self, v: np.ndarray, tau: float, gam2: float) -> np.ndarray:
        v = np.ascontiguousarray(v, dtype=np.float64)
        out = np.zeros(max(self.M, 1))
        check(self._lib.vampomi_lmmse_mult(self.ctx, _dp(v), tau, gam2, _dp(out), MEM_HOST))
        return out[: self.M]

    def pcg(self, v: np.ndarray, tau: float, gam2: float, mu0: Optional[np.ndarray] = None, onsager: bool = False,
            max_iter: int = 500, tol: float = 1e-5):
        v = np.ascontiguousarray(v, dtype=np.float64)
        mu = np.zeros(max(self.M, 1))
        it = C.c_int()
        m0 = None if mu0 is None else np.ascontiguousarray(mu0, dtype=np.float64)
        check(self._lib.vampomi_pcg(self.ctx, _dp(v), None if m0 is None else _dp(m0), tau, gam2,
                                    1 if onsager else 0, max_iter, tol, _dp(mu), C.byref(it), MEM_HOST))
        return mu[: self.M], it.value

    def test_metrics(self, est: np.ndarray):
        """--run-mode test row (src/main_meth.cpp:165-199) for one estimate slice
        (x1_hat / sqrt(N)) on this (test) data set: (R2 test, squared z correlation)."""
        est = np.ascontiguousarray(est, dtype=np.float64)
        if est.shape != (self.M,):
            raise ValueError("estimate slice must have M entries")
        r2, c2 = C.c_double(), C.c_double()
        check(self._lib.vampomi_test_metrics(self.ctx, _dp(est), C.byref(r2), C.byref(c2), MEM_HOST))
        return r2.value, c2.value

    test_metrics.__test__ = False

    def assoc_loo(self, est: np.ndarray, mem_device: bool = False):
        """--pval-method loo (src/main_meth.cpp:245-264, src/data.cpp:385-417).
        est: this shard's estimate-file slice (x1_hat / sqrt(N)).  COLLECTIVE.
        Returns (pvals (M), stats (M, 5): sumx sumsqx sumxy sumy sumsqy)."""
        est = np.ascontiguousarray(est, dtype=np.float64)
        if est.shape != (self.M,):
            raise ValueError("estimate slice must have M entries")
        pv = np.zeros(max(self.M, 1))
        st = np.zeros((max(self.M, 1), 5))
        check(self._lib.vampomi_assoc_loo(self.ctx, _dp(est), _dp(pv), _dp(st), MEM_HOST))
        return pv[: self.M], st[: self.M]

    def assoc_loo_multi(self, Y: np.ndarray, est: Optional[np.ndarray] = None, standardize: bool = True):
        """:meth:`assoc_loo` for T phenotypes with the matrix read once per
        four of them (vampomi_assoc_loo_multi).  Y: (T, N), one phenotype per
        row, each prepared as :meth:`set_phen` prepares it; the context's own
        phenotype is not touched.  est: (T, M) estimate-file slices, or None
        for the plain marginal tests (no A.x pass).  COLLECTIVE.  Returns
        (pvals (T, M), stats (T, M, 5)); block t equals, bit for bit,
        ``set_phen(Y[t], standardize)`` followed by ``assoc_loo(est[t])``."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[1] != self.N:
            raise ValueError("Y must be (T, N)")
        T = Y.shape[0]
        if est is not None:
            est = np.ascontiguousarray(est, dtype=np.float64)
            if est.shape != (T, self.M):
                raise ValueError("estimates must be (T, M)")
            if est.size == 0:  # an empty shard still takes part in the A.x: a non-null pointer
                est = np.zeros(1)
        pv = np.zeros((T, max(self.M, 1)))
        st = np.zeros((T, max(self.M, 1), 5))
        check(self._lib.vampomi_assoc_loo_multi(self.ctx, T, _dp(Y), self.N, 1 if standardize else 0,
                                                None if est is None else _dp(est), _dp(pv), _dp(st), MEM_HOST))
        return pv[:, : self.M], st[:, : self.M]

    def assoc_loco(self, est: Optional[np.ndarray], labels: np.ndarray, G: Optional[int] = None,
                   resid: bool = False):
        """The leave-one-chromosome-out test (vampomi_assoc_loco).  ``labels``:
        the M local markers' labels in [0, G) (``G`` None: max + 1 of the local
        labels, for one rank); marker j is tested marginally against
        ``y_c = (y - z) + z_c``, c = labels[j], the phenotype without the
        fitted effect of every marker outside label c.  ``est``: the
        estimate-file slice (M), or None for all zeros (every y_c is y, no A.x
        pass).  COLLECTIVE.  Two passes over the matrix whatever G is.
        Returns (pvals (M), stats (M, 5)) and with ``resid`` also R (G, N),
        R[c] = y_c."""
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.shape != (self.M,):
            raise ValueError("labels must be (M,)")
        if G is None:
            G = int(labels.max()) + 1 if labels.size else 1
        if est is not None:
            est = np.ascontiguousarray(est, dtype=np.float64)
            if est.shape != (self.M,):
                raise ValueError("estimates must be (M,)")
            if est.size == 0:  # an empty shard still takes part in the all-reduce: a non-null pointer
                est = np.zeros(1)
        if labels.size == 0:
            labels = np.zeros(1, dtype=np.int32)
        pv = np.zeros(max(self.M, 1))
        st = np.zeros((max(self.M, 1), 5))
        R = np.zeros((max(int(G), 1), self.N)) if resid else None
        check(self._lib.vampomi_assoc_loco(self.ctx, None if est is None else _dp(est), _dp(labels), int(G), _dp(pv),
                                           _dp(st), None if R is None else _dp(R), MEM_HOST))
        return (pv[: self.M], st[: self.M], R) if resid else (pv[: self.M], st[: self.M])

    def assoc_se(self, r1: np.ndarray, gam1: float) -> np.ndarray:
        """--pval-method se (src/main_meth.cpp:218-242)."""
        r1 = np.ascontiguousarray(r1, dtype=np.float64)
        pv = np.zeros(max(self.M, 1))
        check(self._lib.vampomi_assoc_se(self.ctx, _dp(r1), gam1, _dp(pv), MEM_HOST))
        return pv[: self.M]

    def update_prior(self, r1: np.ndarray, gam1: float, probs, vars_scaled, EM_max_iter: int = 1,
                     EM_err_thr: float = 1e-2, learn_vars: int = 1, merge_vars_thr: float = 0.5):
        """vamp::updatePrior (src/vamp.cpp:531-643); vars multiplied by N. Returns (probs, vars)."""
        r1 = np.ascontiguousarray(r1, dtype=np.float64)
        L = C.c_int(len(probs))
        pr = np.zeros(MAX_L)
        va_ = np.zeros(MAX_L)
        pr[: L.value] = probs
        va_[: L.value] = vars_scaled
        check(self._lib.vampomi_update_prior(self.ctx, _dp(r1), gam1, C.byref(L), _dp(pr), _dp(va_), EM_max_iter,
                                             EM_err_thr, learn_vars, merge_vars_thr, MEM_HOST))
        return pr[: L.value].copy(), va_[: L.value].copy()

    def denoise_bin(self, p1: np.ndarray, tau1: float, m_cov: Optional[np.ndarray] = None):
        """g1_bin_class / g1d_bin_class over the phenotype (src/vamp_probit.cpp:469-488): (z1, sum of g1d);
        m_cov (N): the covariate offsets Z_i.cov_eff (None: zero, the kernel without an offset)."""
        p1 = np.ascontiguousarray(p1, dtype=np.float64)
        z = np.zeros(self.N)
        sd = C.c_double()
        if m_cov is None:
            check(self._lib.vampomi_denoise_bin(self.ctx, _dp(p1), tau1, _dp(z), C.byref(sd), MEM_HOST))
        else:
            m = np.ascontiguousarray(m_cov, dtype=np.float64)
            if m.shape != (self.N,):
                raise ValueError("m_cov must have N entries")
            check(self._lib.vampomi_denoise_bin_cov(self.ctx, _dp(p1), tau1, _dp(m), _dp(z), C.byref(sd), MEM_HOST))
        return z, sd.value

    def denoise(self, r1: np.ndarray, gam1: float, probs: Sequence[float], vars_scaled: Sequence[float]):
        """(g1(r1), g1d(r1), sum of g1d over ranks); vars already multiplied by N."""
        r1 = np.ascontiguousarray(r1, dtype=np.float64)
        L = len(probs)
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        va = np.ascontiguousarray(vars_scaled, dtype=np.float64)
        x1 = np.zeros(max(self.M, 1))
        x1d = np.zeros(max(self.M, 1))
        s = C.c_double()
        check(self._lib.vampomi_denoise(self.ctx, _dp(r1), gam1, _dp(pr), _dp(va), L, _dp(x1), _dp(x1d),
                                        C.byref(s), MEM_HOST))
        return x1[: self.M], x1d[: self.M], s.value

    # -- measurement --
    def kernel_name(self, which: int, K: int, mode: int = 0) -> str:
        """rocprofv3 name of the kernel this context launches for pass ``which``
        (0 A.x, 1 A^T.u, 2 association test, 3 one-pass CG operator under the
        context's plan)
        with K right-hand sides, under its current variant settings."""
        buf = C.create_string_buffer(256)
        check(self._lib.vampomi_dev_kernel_name(self.ctx, which, K, mode, buf, 256))
        return buf.value.decode()

    def op_apply(self, ar, p, diag: float, tau: float, gam2: float, z=None, qo=None, beta=None):
        """Development hook: one application of the one-pass CG operator on K <= 2
        systems (vampomi_dev_op_apply): returns (d, A d, <d, p>) for
        q = ar/diag [+ beta*qo] and p [= z + beta*p]."""
        ar = np.ascontiguousarray(np.atleast_2d(ar), dtype=np.float64)
        p = np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64)
        K = ar.shape[0]
        if ar.shape != (K, self.N) or p.shape != (K, self.M):
            raise ValueError("ar must be K x N and p K x M")
        fz = z is not None
        if fz:
            z = np.ascontiguousarray(np.atleast_2d(z), dtype=np.float64)
            qo = np.ascontiguousarray(np.atleast_2d(qo), dtype=np.float64)
            beta = np.ascontiguousarray(beta, dtype=np.float64)
        d = np.zeros((K, max(self.M, 1)))
        ad = np.zeros((K, self.N))
        dp = np.zeros(K)
        check(self._lib.vampomi_dev_op_apply(self.ctx, K, _dp(ar), _dp(qo) if fz else None, _dp(p),
                                             _dp(z) if fz else None, _dp(beta) if fz else None, diag, tau, gam2,
                                             _dp(d), _dp(ad), _dp(dp)))
        return d[:, : self.M], ad, dp

    def op_apply3(self, ar, p, diag: float, tau: float, gam2: float, ar3, p3, z=None, qo=None, beta=None):
        """Development hook: one operator launch with three systems
        (vampomi_dev_op_apply3): systems 0 and 1 as op_apply takes them with
        K = 2, and in the third slot the alternate system on ar3 (N) and p3 (M)
        (diag = tau = 1, gam2 = 0, no direction update).  Returns (d, A d,
        <d, p>): 3 x M, 3 x N and the two systems' <d, p>."""
        ar = np.ascontiguousarray(ar, dtype=np.float64)
        p = np.ascontiguousarray(p, dtype=np.float64)
        ar3 = np.ascontiguousarray(ar3, dtype=np.float64)
        p3 = np.ascontiguousarray(p3, dtype=np.float64)
        if ar.shape != (2, self.N) or p.shape != (2, self.M) or ar3.shape != (self.N,) or p3.shape != (self.M,):
            raise ValueError("ar must be 2 x N, p 2 x M, ar3 N and p3 M")
        fz = z is not None
        if fz:
            z = np.ascontiguousarray(z, dtype=np.float64)
            qo = np.ascontiguousarray(qo, dtype=np.float64)
            beta = np.ascontiguousarray(beta, dtype=np.float64)
            if z.shape != (2, self.M) or qo.shape != (2, self.N) or beta.shape != (2,):
                raise ValueError("z must be 2 x M, qo 2 x N and beta 2")
        d = np.zeros((3, max(self.M, 1)))
        ad = np.zeros((3, self.N))
        dp = np.zeros(2)
        check(self._lib.vampomi_dev_op_apply3(self.ctx, _dp(ar), _dp(qo) if fz else None, _dp(p),
                                              _dp(z) if fz else None, _dp(beta) if fz else None, diag, tau, gam2,
                                              _dp(ar3), _dp(p3), _dp(d), _dp(ad), _dp(dp)))
        return d[:, : self.M], ad, dp

    def read_ceiling(self, reps: int = 9) -> dict:
        """The HBM read ceiling on this device for this shard (vampomi_dev_read_ceiling):
        a pure read stream of the resident matrix, the faster variant's median."""
        us, nb, var = C.c_double(), C.c_double(), C.c_int()
        check(self._lib.vampomi_dev_read_ceiling(self.ctx, int(reps), C.byref(us), C.byref(nb), C.byref(var)))
        return {"us_med": us.value, "bytes": nb.value, "GBs": nb.value / (us.value * 1e-6) / 1e9,
                "variant": ("lockstep 8-wave workgroups, one per CU", "1 MiB chunk per wave")[var.value]}

    def set_variant(self, which: int, variant: int):
        """Development hook: this context's kernel variant for pass ``which``."""
        check(self._lib.vampomi_dev_set_variant(self.ctx, which, variant))

    def prestep_counts(self) -> tuple:
        """(made, used): the pre-steps of the linear model's solves since the run began."""
        made, used = C.c_int64(), C.c_int64()
        check(self._lib.vampomi_dev_prestep_counts(self.ctx, C.byref(made), C.byref(used)))
        return made.value, used.value

    def all_ok(self, local_ok: bool) -> bool:
        """COLLECTIVE: True iff local_ok on every rank."""
        out = C.c_int()
        check(self._lib.vampomi_all_ok(self.ctx, 1 if local_ok else 0, C.byref(out)))
        return bool(out.value)

    def comm_abort(self):
        """Poison (loopback) / abort (RCCL) the job's communicator after a local failure."""
        check(self._lib.vampomi_comm_abort(self.ctx))

    def set_timing(self, on: bool = True, period: int = 1):
        """HIP-event timing of the A/A^T launches; period > 1 times one launch
        in `period` of each (kernel class, K) and counts it `period` times."""
        check(self._lib.vampomi_set_timing(self.ctx, (max(1, int(period)) if on else 0)))

    def stats(self) -> Stats:
        s = Stats()
        check(self._lib.vampomi_get_stats(self.ctx, C.byref(s)))
        return s

    def reset_stats(self):
        check(self._lib.vampomi_reset_stats(self.ctx))


@dataclass
class VampOptions:
    """Hyper-parameters of vamp::vamp (defaults: src/options.hpp:62-104)."""
    gam1: float = 1e-6
    h2: float = 0.5
    max_iter: int = 50
    CG_max_iter: int = 500
    CG_err_tol: float = 1e-5
    EM_max_iter: int = 1
    EM_err_thr: float = 1e-2
    rho: float = 0.5
    learn_vars: int = 1
    learn_prior_delay: int = 1
    stop_criteria_thr: float = 0.01
    merge_vars_thr: float = 0.5
    vars: Sequence[float] = (0, 1e-06, 6e-06, 3e-05, 2e-04, 1e-03, 6e-03, 3e-02, 2e-01, 1e+00)
    probs: Sequence[float] = (9.9e-01, 5e-03, 2.5e-03, 1.25e-03, 6.25e-04, 3.125e-04, 1.5625e-04, 7.8125e-05,
                              3.90625e-05, 3.90625e-05)
    seed: int = 0x5EED5EED
    out_dir: str = ""
    out_name: str = ""
    verbosity: int = 0
    batch_rhs: int = 4
    model: str = "linear"

    def to_struct(self) -> Params:
        p = Params()
        load().vampomi_params_default(C.byref(p))
        for k in ("gam1", "h2", "max_iter", "CG_max_iter", "CG_err_tol", "EM_max_iter", "EM_err_thr", "rho",
                  "learn_vars", "learn_prior_delay", "stop_criteria_thr", "merge_vars_thr", "seed", "verbosity",
                  "batch_rhs"):
            setattr(p, k, getattr(self, k))
        if len(self.vars) != len(self.probs) or not 1 <= len(self.vars) <= MAX_L:
            raise ValueError("vars and probs must have the same length (1..64)")
        p.L = len(self.vars)
        for j, (v, q) in enumerate(zip(self.vars, self.probs)):
            p.vars[j] = v
            p.probs[j] = q
        self._keep = [self.out_dir.encode(), self.out_name.encode(), self.model.encode()]
        p.out_dir, p.out_name, p.model = self._keep
        return p


class Vamp:
    """The reference's ``class vamp``: ``Vamp(data, opts).infere(...)``."""

    def __init__(self, data: Data, opts: Optional[VampOptions] = None, true_signal: Optional[np.ndarray] = None,
                 x1hat_init: Optional[np.ndarray] = None):
        self.data = data
        self.opts = opts or VampOptions()
        self.true_signal = None if true_signal is None else np.ascontiguousarray(true_signal, dtype=np.float64)
        self.x1hat_init = None if x1hat_init is None else np.ascontiguousarray(x1hat_init, dtype=np.float64)
        self._active = False

    def _prepare(self, keep_hist: bool):
        o, M = self.opts, self.data.M
        it = o.max_iter
        self.p = o.to_struct()
        if self.true_signal is not None:
            self.p.true_signal = self.true_signal.ctypes.data
        if self.x1hat_init is not None:
            self.p.x1hat_init = self.x1hat_init.ctypes.data
        self.cg = np.zeros(it, dtype=np.int32)
        self.ons = np.zeros(it, dtype=np.int32)
        self.Lh = np.zeros(it, dtype=np.int32)
        probit = o.model == "bin_class"
        self.params = np.zeros((it, 8 if probit else 5))
        self.metrics = np.zeros((it, 12 if probit else 6))
        self.prior = np.zeros((it, 1 + 2 * MAX_L)) if probit else None
        self.x1_final = np.zeros(max(M, 1))
        r = Result()
        ip = C.POINTER(C.c_int)
        r.cg_iters = self.cg.ctypes.data_as(ip)
        r.ons_iters = self.ons.ctypes.data_as(ip)
        r.L_hist = self.Lh.ctypes.data_as(ip)
        r.params = self.params.ctypes.data_as(C.POINTER(C.c_double))
        r.metrics = self.metrics.ctypes.data_as(C.POINTER(C.c_double))
        r.x1_final = self.x1_final.ctypes.data_as(C.POINTER(C.c_double))
        if self.prior is not None:
            r.prior_hist = self.prior.ctypes.data_as(C.POINTER(C.c_double))
        if keep_hist:
            self.x1_hist = np.zeros((it, max(M, 1)))
            self.r1_hist = np.zeros((it, max(M, 1)))
            r.x1_hist = self.x1_hist.ctypes.data_as(C.POINTER(C.c_double))
            r.r1_hist = self.r1_hist.ctypes.data_as(C.POINTER(C.c_double))
        self.r = r

    def infere(self, keep_hist: bool = False) -> np.ndarray:
        """Run vamp::infere to completion; returns what it returns (local slice):
        x1_hat / sqrt(N) for the linear model, x1_hat for bin_class."""
        self._prepare(keep_hist)
        check(load().vampomi_infere(self.data.ctx, C.byref(self.p), C.byref(self.r)))
        return self.x1_final[: self.data.M].copy()

    # step-wise API (one VAMP iteration per step)
    def begin(self, keep_hist: bool = False):
        self._prepare(keep_hist)
        check(load().vampomi_vamp_begin(self.data.ctx, C.byref(self.p), C.byref(self.r)))
        self._active = True

    def step(self) -> bool:
        s = C.c_int()
        check(load().vampomi_vamp_step(self.data.ctx, C.byref(s)))
        return bool(s.value)

    def step_phases(self):
        """The last step's (solves, whole step) seconds as the host sees them
        (vampomi_step_phases; the reference's "CG took" / "Total iteration time")."""
        a, b = C.c_double(), C.c_double()
        check(load().vampomi_step_phases(self.data.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def end(self) -> np.ndarray:
        check(load().vampomi_vamp_end(self.data.ctx))
        self._active = False
        return self.x1_final[: self.data.M].copy()

    @property
    def cov_eff(self) -> np.ndarray:
        """The covariate effects fitted at the start of this context's last
        bin_class run (C entries; empty without covariates)."""
        C_ = getattr(self.data, "C", 0)
        out = np.zeros(max(C_, 1))
        check(load().vampomi_get_cov_eff(self.data.ctx, _dp(out)))
        return out[:C_]

    def probit_state(self):
        """(p1 (N), tau1) that the next step's z-side denoiser reads (bin_class, between begin and end)."""
        p1 = np.zeros(self.data.N)
        t = C.c_double()
        check(load().vampomi_get_probit_state(self.data.ctx, _dp(p1), C.byref(t)))
        return p1, t.value

    @property
    def iterations_run(self) -> int:
        return self.r.iterations_run

    @property
    def a_passes(self):
        return self.r.a_passes_ref, self.r.a_passes_exec

    def summary(self) -> dict:
        n = self.r.iterations_run
        return {
            "iterations": n,
            "cg_iters": self.cg[:n].tolist(),
            "ons_iters": self.ons[:n].tolist(),
            "L": self.Lh[:n].tolist(),
            "params": self.params[:n].tolist(),
            "metrics": self.metrics[:n].tolist(),
            "a_passes_ref": self.r.a_passes_ref,
            "a_passes_exec": self.r.a_passes_exec,
            **({"prior": self.prior[:n].tolist()} if self.prior is not None else {}),
        }
