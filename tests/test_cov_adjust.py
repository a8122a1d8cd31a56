"""Covariate adjustment without a device: the ABI additions, the basis of
vampomi_adjust_basis against numpy, and the CLI's checks of --cov-adjust, which
all end before the context is opened.  (vampomi_set_adjust needs an open
context, which needs a device: tests/test_gpu_cov_adjust.py.)"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _cov_adjust as H
import vampomi_amd as va
from vampomi_amd import _lib


def test_symbols_and_abi_version():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("vampomi_adjust_basis", "vampomi_set_adjust", "vampomi_read_adjust", "vampomi_get_adjust",
                 "vampomi_get_adjust_stats"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert va.load().vampomi_abi_version() == 3
    assert "adjust_basis" in va.__all__


@pytest.mark.parametrize("n,nc", [(301, 0), (301, 1), (301, 5), (2049, 64)], ids=lambda v: str(v))
def test_basis(n, nc):
    Z, planted = H.covariates(n, nc)
    Q, dropped = va.adjust_basis(Z)
    assert dropped.dtype == bool and dropped.tolist() == planted.tolist()  # exactly the planted columns
    R = 1 + nc - int(planted.sum())
    assert Q.shape == (n, R)
    err = np.abs(Q.T @ Q - np.eye(R)).max()
    print("max |Q^T Q - I| = %.3e at %d x %d" % (err, n, nc))
    assert err <= 1e-13
    assert np.all(np.abs(np.abs(Q[:, 0]) - 1 / np.sqrt(n)) <= 4e-16 / np.sqrt(n)) and len(np.unique(Q[:, 0])) == 1
    # the span is numpy's: the same rank, Q inside span{1, Z}, and {1, Z} inside span Q
    Z1 = H.design(Z)
    assert np.linalg.matrix_rank(Z1) == R
    assert np.abs(H.residual(H.design(Z, planted), Q)).max() <= 1e-12
    assert np.abs(Z1 - Q @ (Q.T @ Z1)).max() <= 1e-12
    # the order is the file's: column k of Q lies in the span of the intercept and the first kept columns
    kept = np.flatnonzero(~planted)
    for k in range(1, min(R, 4)):
        lead = H.design(Z[:, kept[:k]])
        assert np.abs(H.residual(lead, Q[:, k])).max() <= 1e-12


def test_basis_argument_errors():
    lib = va.load()
    R = C.c_int(-1)
    Q = np.zeros((3, 10))
    Z = np.ones((2, 10))
    d = np.zeros(2, dtype=np.int32)

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    assert lib.vampomi_adjust_basis(p(Z), 10, 65, 10, p(Q), C.byref(R), p(d)) == 1  # C > VAMPOMI_MAX_C
    assert lib.vampomi_adjust_basis(p(Z), 10, -1, 10, p(Q), C.byref(R), p(d)) == 1
    assert lib.vampomi_adjust_basis(p(Z), 10, 2, 9, p(Q), C.byref(R), p(d)) == 1  # ld_in < n
    assert lib.vampomi_adjust_basis(None, 10, 2, 10, p(Q), C.byref(R), p(d)) == 1
    Z[1, 4] = np.nan
    assert lib.vampomi_adjust_basis(p(Z), 10, 2, 10, p(Q), C.byref(R), p(d)) == 1
    assert b"covariate 1, row 4 is not finite" in lib.vampomi_last_error()
    assert lib.vampomi_adjust_basis(None, 10, 0, 10, p(Q), C.byref(R), None) == 0 and R.value == 1
    assert np.all(Q[0] == 1 / np.sqrt(10))
    with pytest.raises(ValueError):
        va.adjust_basis(np.ones(5))


def test_data_rejects_adjust_C_without_a_path_before_opening_a_context():
    with pytest.raises(ValueError):
        va.Data(10, 4, adjust=np.ones((10, 1)), adjust_C=1)
    with pytest.raises(ValueError):
        va.Data(10, 4, adjust="some.cov")
    with pytest.raises(ValueError):
        va.Data(10, 4, adjust_C=2)


# ---- CLI: all of these end before the device is opened -------------------------------
def cli(*args):
    return subprocess.run([va.CLI_PATH, "--N", "12", "--Mt", "20", "--meth-file", "absent.bin", *args],
                          capture_output=True, text=True, timeout=120)


def _fatal(r, text):
    assert r.returncode == 1, r.stdout
    assert text in r.stdout and "cannot open the device context" not in r.stdout, r.stdout


def test_cli_residual_needs_the_linear_model():
    _fatal(cli("--cov-adjust", "residual", "--model", "bin_class", "--C", "2", "--cov-file", "absent.cov"),
           "FATAL  : option --cov-adjust residual needs --model linear!")


def test_cli_residual_needs_a_cov_file_and_C():
    _fatal(cli("--cov-adjust", "residual", "--C", "2"), "FATAL  : option --cov-adjust residual needs --cov-file!")
    _fatal(cli("--cov-adjust", "residual", "--cov-file", "absent.cov"),
           "FATAL  : option --cov-adjust residual needs --C of at least 1!")


def test_cli_value_is_checked():
    _fatal(cli("--cov-adjust", "regress"),
           "FATAL  : option --cov-adjust has to be none or residual! (regress was passed)")


def test_cli_test_mode_needs_the_test_table():
    _fatal(cli("--cov-adjust", "residual", "--C", "2", "--cov-file", "absent.cov", "--run-mode", "test"),
           "FATAL  : option --cov-adjust residual needs --cov-file-test in --run-mode test!")


def test_cli_u16_storage_cannot_hold_residuals():
    _fatal(cli("--cov-adjust", "residual", "--C", "2", "--cov-file", "absent.cov", "--meth-storage", "u16"),
           "FATAL  : option --cov-adjust residual cannot be held by --meth-storage u16")


def test_cli_a_table_that_does_not_parse_ends_the_run(tmp_path):
    p = tmp_path / "short.cov"
    H.write_cov(p, np.ones((12, 1)))  # one column where --C says two
    _fatal(cli("--cov-adjust", "residual", "--C", "2", "--cov-file", str(p)), "FATAL  : covariate adjustment: ")
    _fatal(cli("--cov-adjust", "residual", "--C", "2", "--cov-file", str(tmp_path / "absent.cov")),
           "FATAL  : covariate adjustment: ")


def test_cli_none_is_the_default_and_keeps_the_ignored_line_out_of_the_parser():
    r = subprocess.run([va.CLI_PATH, "--N", "12", "--Mt", "20", "--cov-adjust", "none"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "no meth file provided" in r.stdout and "--cov-adjust" not in r.stdout, r.stdout
