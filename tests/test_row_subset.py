"""Row subsets without a device: the ABI additions, the kept-rows reader
(vampomi_phen_rows: a PLINK phenotype file, a --keep style list, NA rows) and
the CLI's checks, which run on the host before the context is opened."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vampomi_amd as va
from vampomi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NA_ROWS = (3, 9)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A 12-row phenotype file with NA at rows 3 and 9, and keep files."""
    d = tmp_path_factory.mktemp("rows")
    phen = d / "y.phen"
    with open(phen, "w") as f:
        for i in range(12):
            f.write("fam%d id%d %s\n" % (i // 4, i, "NA" if i in NA_ROWS else "%0.10f" % (0.25 * i - 1)))
    keep = d / "keep.txt"  # shuffled, a duplicate line, further fields, a blank line; names NA row 9
    keep.write_text("fam2 id11\nfam0 id0 extra fields\nfam2 id9\n\nfam1 id5\nfam0 id2\nfam1 id5\nfam1 id7\n")
    clean = d / "clean.txt"  # omits both NA rows
    clean.write_text("fam1 id4\nfam0 id1\nfam2 id10\n")
    unknown = d / "unknown.txt"
    unknown.write_text("fam0 id1\nfam7 id77\n")
    return {"dir": d, "phen": str(phen), "keep": str(keep), "clean": str(clean), "unknown": str(unknown)}


def phen_rows_raw(phen, keep, drop_na, cap=None, count_only=False):
    lib = va.load()
    nf, n = C.c_int64(-1), C.c_int64(-1)
    rows = np.full(16 if cap is None else max(cap, 1), -1, dtype=np.int64)
    st = lib.vampomi_phen_rows(phen.encode(), None if keep is None else keep.encode(), drop_na,
                               None if count_only else rows.ctypes.data_as(C.c_void_p),
                               len(rows) if cap is None else cap, C.byref(nf), C.byref(n))
    return st, rows, nf.value, n.value


def test_symbols_and_abi_version():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("vampomi_set_row_subset", "vampomi_get_row_subset", "vampomi_phen_rows"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert va.load().vampomi_abi_version() == 3


def test_keep_file_and_drop_na(files):
    st, rows, nf, n = phen_rows_raw(files["phen"], files["keep"], 1)
    assert (st, nf, n) == (0, 12, 5)
    assert rows[:n].tolist() == [0, 2, 5, 7, 11]  # file order, the duplicate once, NA row 9 dropped
    r, N_file = va.phen_rows(files["phen"], keep_file=files["keep"], drop_na=True)
    assert r.tolist() == [0, 2, 5, 7, 11] and N_file == 12 and r.dtype == np.int64


def test_na_in_a_kept_row_is_fatal_without_drop(files):
    st, _, _, _ = phen_rows_raw(files["phen"], files["keep"], 0)
    assert st == 5 and b"NAN in data!" in va.load().vampomi_last_error()
    with pytest.raises(va.VampomiError) as e:
        va.phen_rows(files["phen"], keep_file=files["keep"])
    assert e.value.status == 5


def test_na_only_in_dropped_rows_is_accepted(files):
    st, rows, nf, n = phen_rows_raw(files["phen"], files["clean"], 0)
    assert (st, nf, n) == (0, 12, 3) and rows[:n].tolist() == [1, 4, 10]


def test_no_keep_file(files):
    st, rows, nf, n = phen_rows_raw(files["phen"], None, 1)
    assert (st, nf, n) == (0, 12, 10) and rows[:n].tolist() == [i for i in range(12) if i not in NA_ROWS]
    assert phen_rows_raw(files["phen"], None, 0)[0] == 5


def test_unknown_pair_names_the_pair(files):
    st, _, _, _ = phen_rows_raw(files["phen"], files["unknown"], 1)
    msg = va.load().vampomi_last_error().decode()
    assert st == 1 and "fam7 id77" in msg and "line 2" in msg


def test_missing_files(files):
    assert phen_rows_raw(str(files["dir"] / "absent.phen"), None, 1)[0] == 4
    assert phen_rows_raw(files["phen"], str(files["dir"] / "absent.txt"), 1)[0] == 4


def test_count_only_and_small_cap(files):
    st, _, nf, n = phen_rows_raw(files["phen"], files["keep"], 1, count_only=True)
    assert (st, nf, n) == (0, 12, 5)
    st, rows, _, _ = phen_rows_raw(files["phen"], files["keep"], 1, cap=4)
    assert st == 1 and rows.tolist() == [-1] * 4  # nothing written
    assert phen_rows_raw(files["phen"], files["keep"], 1, cap=5)[0] == 0


# ---- CLI: all of these end before the device is opened ----
def cli(*args):
    return subprocess.run([va.CLI_PATH, "--meth-file", "absent.bin", "--N", "12", "--Mt", "20", *args],
                          capture_output=True, text=True, timeout=120)


def test_cli_phen_na_value_is_checked(files):
    r = cli("--phen-file", files["phen"], "--phen-na", "maybe")
    assert r.returncode == 1 and "FATAL" in r.stdout and "--phen-na" in r.stdout and "(maybe was passed)" in r.stdout


def test_cli_keep_file_with_an_absent_id_is_fatal(files):
    r = cli("--phen-file", files["phen"], "--keep-file", files["unknown"], "--phen-na", "drop")
    assert r.returncode == 1 and "FATAL" in r.stdout and "fam7 id77" in r.stdout
    assert "cannot open the device context" not in r.stdout


def test_cli_na_under_the_default_is_fatal_with_the_reference_text(files):
    r = cli("--phen-file", files["phen"], "--keep-file", files["keep"])
    assert r.returncode == 1 and "FATAL" in r.stdout and "NAN in data!" in r.stdout
    assert "cannot open the device context" not in r.stdout


def test_cli_fewer_than_two_kept_rows_is_fatal(files):
    one = files["dir"] / "one.txt"
    one.write_text("fam0 id1\n")
    r = cli("--phen-file", files["phen"], "--keep-file", str(one))
    assert r.returncode == 1 and "FATAL" in r.stdout and "1 of 12 samples" in r.stdout


def test_cli_reports_the_kept_rows_before_opening_the_device(files):
    r = cli("--phen-file", files["phen"], "--keep-file", files["keep"], "--phen-na", "drop")
    assert "INFO   : kept 5 of 12 samples (6 not in the keep file, 1 with an NA phenotype)" in r.stdout


def test_sanitized_host_parsers(files, tmp_path):
    """The new host parsers under AddressSanitizer and UBSan, in a stand-alone
    program (tests/phen_rows_harness.cpp), on the files above and on malformed
    ones."""
    exe = tmp_path / "phen_rows_harness"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vampomi_amd", "csrc"), os.path.join(ROOT, "tests", "phen_rows_harness.cpp"),
                    os.path.join(ROOT, "vampomi_amd", "csrc", "hostio.cpp"), "-o", str(exe)], check=True)

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout.split()

    assert run(files["phen"], files["keep"], 1) == ["0", "12", "6", "1", "0", "2", "5", "7", "11"]
    assert run(files["phen"], files["keep"], 0)[0] == "-2"
    assert run(files["phen"], "-", 1)[:4] == ["0", "12", "0", "2"]
    assert run(files["phen"], files["unknown"], 1)[0] == "-3"
    assert run(tmp_path / "absent", "-", 1)[0] == "-1"
    odd = tmp_path / "odd.phen"  # short lines, leading blanks (an empty first token), no final newline, CRLF
    odd.write_text("\n a b 1\nx y\n   \nfam id NA\r\nfam id2 3.5 more\t\n\tq")
    assert run(odd, "-", 1) == ["0", "3", "0", "1", "0", "2"]
    oddkeep = tmp_path / "odd.keep"
    oddkeep.write_text("\n\t\nfam id2\r\n a\n")  # " a" splits into "" and "a": the pair of row 0
    assert run(odd, oddkeep, 1) == ["0", "3", "1", "0", "0", "2"]
    bad = tmp_path / "bad.keep"
    bad.write_text("lonely\n")
    assert run(odd, bad, 1)[0] == "-3"
