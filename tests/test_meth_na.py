"""Missing methylation values without a device: the ABI additions, the CLI's
checks of --meth-na / --meth-na-max-frac (host-side, before the context is
opened) and the numpy restatement of the fill (tests/_meth_na.py) against
columns worked out by hand.  (vampomi_set_meth_na needs an open context, which
needs a device: its argument checks are in tests/test_gpu_meth_na.py.)"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import _meth_na as H
import vampomi_amd as va
from vampomi_amd import _lib


def test_symbols_status_and_abi_version():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("vampomi_set_meth_na", "vampomi_get_meth_na", "vampomi_get_missing_stats"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert va.load().vampomi_abi_version() == 3
    assert _lib.STATUS[10] == "ERR_NAN_METH" and _lib.STATUS[9] == "ERR_RANGE"
    assert (_lib.NA_PASS, _lib.NA_FATAL, _lib.NA_MEAN) == (0, 1, 2)
    assert str(va.VampomiError(10, "x")) == "ERR_NAN_METH: x"


def test_data_rejects_bad_policy_arguments_before_opening_a_context():
    with pytest.raises(ValueError):
        va.Data(10, 4, meth_na="median")
    for policy in (None, "pass", "fatal"):  # as on the command line: the fraction belongs to "mean"
        with pytest.raises(ValueError):
            va.Data(10, 4, meth_na=policy, max_missing_frac=0.5)


# ---- CLI: all of these end before the device is opened -------------------------------
def cli(*args):
    return subprocess.run([va.CLI_PATH, "--N", "12", "--Mt", "20", *args], capture_output=True, text=True, timeout=120)


def test_cli_meth_na_value_is_checked():
    r = cli("--meth-file", "absent.bin", "--meth-na", "median")
    assert r.returncode == 1
    assert "FATAL  : option --meth-na has to be pass, fatal or mean! (median was passed)" in r.stdout


@pytest.mark.parametrize("bad", ["1.5", "-0.1", "nan", "half", "0.5x", ""])
def test_cli_max_frac_value_is_checked(bad):
    r = cli("--meth-file", "absent.bin", "--meth-na", "mean", "--meth-na-max-frac", bad)
    assert r.returncode == 1, r.stdout
    assert "FATAL  : option --meth-na-max-frac has to be a number in [0, 1]! (%s was passed)" % bad in r.stdout


@pytest.mark.parametrize("policy", [(), ("--meth-na", "pass"), ("--meth-na", "fatal")], ids=["unset", "pass", "fatal"])
def test_cli_max_frac_needs_mean(policy):
    for args in ((*policy, "--meth-na-max-frac", "0.2"), ("--meth-na-max-frac", "0.2", *policy)):  # either order
        r = cli("--meth-file", "absent.bin", *args)
        assert r.returncode == 1 and "FATAL  : option --meth-na-max-frac needs --meth-na mean!" in r.stdout, r.stdout
        assert "cannot open the device context" not in r.stdout


@pytest.mark.parametrize("args", [("--meth-na", "pass"), ("--meth-na", "fatal"), ("--meth-na", "mean"),
                                  ("--meth-na", "mean", "--meth-na-max-frac", "0"),
                                  ("--meth-na-max-frac", "1", "--meth-na", "mean"),
                                  ("--meth-na", "mean", "--meth-na-max-frac", "2.5e-1")], ids=lambda a: "_".join(a))
def test_cli_accepted_values_pass_the_parser(args):
    """Accepted: the parser goes on to its next check, the one for a missing
    --meth-file, and the flags are echoed nowhere as FATAL."""
    r = cli(*args)
    assert r.returncode == 1 and "no meth file provided" in r.stdout and "--meth-na" not in r.stdout, r.stdout


# ---- the numpy helper against columns worked out by hand -------------------------------
def test_fill_reference_by_hand():
    nan = np.nan
    X = np.array([[0.25, nan, 0.75, 0.5],      # one missing of four: mean 0.5
                  [nan, nan, nan, 0.125],      # three of four
                  [nan, nan, nan, nan],        # no observed entry
                  [0.5, 0.25, 1.0, 0.0]])      # none
    r = H.fill_reference(X, 1.0)
    assert r["counts"].tolist() == [1, 3, 4, 0] and r["masked"].tolist() == [False, False, True, False]
    assert r["mean"].tolist() == [0.5, 0.125, 0.0, 0.4375]
    assert r["stats"] == {"missing": 8, "markers_with_missing": 3, "markers_masked": 1}
    assert r["gamma"][0] == 4 * 2.0 ** -53 * 0.5 and r["gamma"][2] == 0
    # the threshold is strict: 1 of 4 is not more than 0.25 of them, 3 of 4 is
    assert H.fill_reference(X, 0.25)["masked"].tolist() == [False, True, True, False]
    assert H.fill_reference(X, 0.2499)["masked"].tolist() == [True, True, True, False]
    # 0.0 masks every marker that has a missing entry and no other
    assert H.fill_reference(X, 0.0)["masked"].tolist() == [True, True, True, False]
    assert H.fill_reference(X, 0.75)["masked"].tolist() == [False, False, True, False]


def test_fsum_mean_is_the_exact_one():
    x = np.array([1.0, 2.0 ** -60, -1.0, np.nan, 2.0 ** -60])  # a naive left-to-right sum loses the small terms
    r = H.fill_reference(x[None, :])
    assert r["mean"][0] == 2.0 ** -59 / 4 and r["counts"][0] == 1
    assert r["gamma"][0] == 5 * 2.0 ** -53 * ((2 + 2.0 ** -59) / 4)


def test_conv_is_the_storage_rule():
    v = np.array([0.0, 0.5, 1.0, 1 - 2.0 ** -17, 2.0 ** -17, 3 * 2.0 ** -17, 0.1])
    assert np.array_equal(H.conv(v, "f64"), v)
    assert H.conv(v, "u16").tolist() == [0.0, 0.5, 65535 / 65536, 65535 / 65536, 0.0, 2 / 65536,
                                         np.rint(0.1 * 65536) / 65536]  # ties to even, 1.0 clamped
    assert H.conv(0.1, "f32") == float(np.float32(0.1)) != 0.1
    assert H.conv(-1e-20, "u16") == 0.0 and H.conv(1 + 1e-12, "u16") == 65535 / 65536  # a bound taken back in


def test_planted_patterns():
    N, M = 301, 12
    mask = H.plant_mask(N, M)
    assert mask.shape == (M, N)
    assert mask.sum(axis=1)[:8].tolist() == [0, 1, 1, 129, 151, 300, 301, 5]
    assert mask[1, 0] and mask[2, N - 1] and not mask[5, N // 2]
    assert mask[3, 10:74].all() and not mask[3, 74:100].any() and mask[3, 100:165].all()
    assert np.all(mask.sum(axis=1)[8:] == 2)  # 0.5 % of 301
    assert np.array_equal(mask, H.plant_mask(N, M))  # a fixed seed
    X = np.linspace(0, 1, N * M).reshape(M, N)
    for dt in (np.float64, np.float32):
        Xin = H.with_nans(X, mask, dt)
        assert Xin.dtype == dt and np.array_equal(np.isnan(Xin), mask)
        assert np.array_equal(Xin[~mask], X.astype(dt)[~mask])
        bits = Xin.view(np.uint64 if dt == np.float64 else np.uint32)[mask]
        assert len(np.unique(bits)) == 6  # every kind of NaN is there, signs and payloads included
        assert np.signbit(Xin[mask]).any() and not np.signbit(Xin[mask]).all()


def test_check_filled_accepts_the_rule_and_rejects_a_wrong_fill():
    N, M = 301, 10
    rng = np.random.default_rng(1)
    X = rng.random((M, N))
    mask = H.plant_mask(N, M)
    Xin = H.with_nans(X, mask, np.float64)
    for storage in ("f64", "f32", "u16"):
        ref = H.fill_reference(Xin)
        plain = H.conv(np.where(mask, 0.5, X), storage)
        stored = np.where(mask, H.conv(ref["mean"], storage)[:, None], plain)
        stored[ref["masked"]] = 0.0
        H.check_filled(stored, plain, Xin, storage)
        bad = stored.copy()
        bad[4, 0] += 2.0 ** -15  # (marker 4: every second row, row 0 missing) two grid steps off
        with pytest.raises(AssertionError):
            H.check_filled(bad, plain, Xin, storage)
        bad = stored.copy()
        bad[1, 7] = 0.5  # an observed entry changed
        with pytest.raises(AssertionError):
            H.check_filled(bad, plain, Xin, storage)
