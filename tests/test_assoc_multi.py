"""Several phenotypes in one pass, without a device: the ABI additions
(vampomi_assoc_loo_multi, vampomi_phen_rows_common), the common kept rows of
several phenotype files, and the checks of --trait-file, which all end on the
host before the context is opened."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import vampomi_amd as va
from vampomi_amd import _lib

NA = {0: (), 1: (3, 9), 2: (9, 10)}  # NA rows of the three files


def _write_phen(path, na=(), ids=None, n=12):
    ids = ids or [("fam%d" % (i // 4), "id%d" % i) for i in range(n)]
    with open(path, "w") as f:
        for i, (a, b) in enumerate(ids):
            f.write("%s %s %s\n" % (a, b, "NA" if i in na else "%0.10f" % (0.25 * i - 1)))
    return ids


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("multi")
    out = {"dir": d, "phen": []}
    for t in range(3):
        p = d / ("y%d.phen" % t)
        ids = _write_phen(p, NA[t])
        out["phen"].append(str(p))
    keep = d / "keep.txt"  # shuffled, a duplicate line, further fields, a blank line; names NA rows 9 and 10
    keep.write_text("fam2 id11\nfam0 id0 extra fields\nfam2 id9\n\nfam1 id5\nfam0 id2\nfam2 id10\nfam1 id5\nfam1 id7\n")
    out["keep"] = str(keep)
    short = d / "short.phen"
    _write_phen(short, n=11)
    out["short"] = str(short)
    swapped = d / "swapped.phen"
    ids[6], ids[7] = ids[7], ids[6]
    _write_phen(swapped, ids=ids)
    out["swapped"] = str(swapped)
    return out


def test_symbols_abi_version_and_stats_layout():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("vampomi_assoc_loo_multi", "vampomi_phen_rows_common"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert va.load().vampomi_abi_version() == 3
    # vampomi_stats keeps its layout: 17 kernel records of 48 bytes and two counters
    assert C.sizeof(_lib.KernelStat) == 48 and C.sizeof(_lib.Stats) == 17 * 48 + 16
    assert _lib.Stats.loo.offset == 10 * 48 + 16
    assert hasattr(va.Data, "assoc_loo_multi") and "phen_rows_common" in va.__all__


@pytest.mark.parametrize("t", [0, 1])
@pytest.mark.parametrize("keep", [False, True])
def test_one_file_is_phen_rows(files, t, keep):
    kf = files["keep"] if keep else None
    r1, n1 = va.phen_rows(files["phen"][t], keep_file=kf, drop_na=True)
    rc, nc, na = va.phen_rows_common([files["phen"][t]], keep_file=kf, drop_na=True)
    assert np.array_equal(r1, rc) and n1 == nc == 12 and rc.dtype == np.int64
    kept = [0, 2, 5, 7, 9, 10, 11] if keep else list(range(12))
    assert na.tolist() == [len(set(NA[t]) & set(kept))]
    if NA[t] and (not keep or set(NA[t]) & set(kept)):
        for call in (lambda: va.phen_rows(files["phen"][t], keep_file=kf),
                     lambda: va.phen_rows_common([files["phen"][t]], keep_file=kf)):
            with pytest.raises(va.VampomiError) as e:
                call()
            assert e.value.status == 5 and "NAN in data!" in str(e.value)


def test_intersection_under_drop_na(files):
    rows, nf, na = va.phen_rows_common(files["phen"], drop_na=True)
    assert rows.tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 11] and nf == 12 and na.tolist() == [0, 2, 2]
    # the keep file: file order, the duplicate once, further fields ignored; it names NA rows 9 (twice NA) and 10
    rows, nf, na = va.phen_rows_common(files["phen"], keep_file=files["keep"], drop_na=True)
    assert rows.tolist() == [0, 2, 5, 7, 11] and nf == 12 and na.tolist() == [0, 1, 2]
    rows, _, na = va.phen_rows_common(files["phen"][:2], keep_file=files["keep"], drop_na=True)
    assert rows.tolist() == [0, 2, 5, 7, 10, 11] and na.tolist() == [0, 1]


def test_na_without_drop_names_the_file(files):
    with pytest.raises(va.VampomiError) as e:
        va.phen_rows_common(files["phen"])
    assert e.value.status == 5 and "NAN in data!" in str(e.value) and "y1.phen" in str(e.value)
    with pytest.raises(va.VampomiError) as e:
        va.phen_rows_common([files["phen"][0], files["phen"][2]], keep_file=files["keep"])
    assert e.value.status == 5 and "y2.phen" in str(e.value)
    rows, _, na = va.phen_rows_common([files["phen"][0], files["phen"][0]])
    assert rows.tolist() == list(range(12)) and na.tolist() == [0, 0]


def test_differing_files_are_an_argument_error(files):
    with pytest.raises(va.VampomiError) as e:
        va.phen_rows_common([files["phen"][0], files["phen"][1], files["short"]], drop_na=True)
    assert e.value.status == 1 and "short.phen" in str(e.value) and "11 rows" in str(e.value)
    with pytest.raises(va.VampomiError) as e:
        va.phen_rows_common([files["phen"][0], files["swapped"], files["short"]], drop_na=True)
    assert e.value.status == 1 and "swapped.phen" in str(e.value) and "row 7" in str(e.value)
    lib = va.load()
    assert lib.vampomi_phen_rows_common(None, 0, None, 0, None, 0, None, None, None) == 1


def test_count_only_and_small_cap(files):
    lib = va.load()
    arr = (C.c_char_p * 3)(*[p.encode() for p in files["phen"]])
    nf, n = C.c_int64(-1), C.c_int64(-1)
    assert lib.vampomi_phen_rows_common(arr, 3, None, 1, None, 0, C.byref(nf), C.byref(n), None) == 0
    assert (nf.value, n.value) == (12, 9)
    rows = np.full(8, -1, dtype=np.int64)
    assert lib.vampomi_phen_rows_common(arr, 3, None, 1, rows.ctypes.data_as(C.c_void_p), 8, None, None, None) == 1
    assert rows.tolist() == [-1] * 8  # nothing written


# ---- CLI: all of these end before the device is opened ----
def cli(*args):
    return subprocess.run([va.CLI_PATH, "--meth-file", "absent.bin", "--N", "12", "--Mt", "20", "--out-dir", ".",
                           *args], capture_output=True, text=True, timeout=120)


LOO = ("--run-mode", "association_test", "--pval-method", "loo")


@pytest.fixture(scope="module")
def traits(files):
    d = files["dir"]
    good = d / "traits.txt"
    good.write_text("# name phen estimate\n\n" + "".join(
        "t%d %s %s\n" % (t, files["phen"][t], d / ("e%d_it_7.bin" % t)) for t in range(3)))
    return {"good": str(good), "dir": d}


def _fatal(r, *words):
    assert r.returncode == 1, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("FATAL")]
    assert len(lines) == 1 and all(w in lines[0] for w in words), r.stdout
    assert "cannot open the device context" not in r.stdout


@pytest.mark.parametrize("extra,word", [(("--phen-file", "y.phen"), "--phen-file"),
                                        (("--estimate-file", "e_it_3.bin"), "--estimate-file"),
                                        (("--r1-file", "r1_it_3.bin"), "--r1-file")])
def test_cli_trait_file_excludes_the_single_phenotype_flags(traits, extra, word):
    _fatal(cli(*LOO, "--trait-file", traits["good"], *extra), "--trait-file", word)


@pytest.mark.parametrize("mode,why", [(("--run-mode", "infere"), "needs --run-mode association_test"),
                                      (("--run-mode", "test"), "needs --run-mode association_test"),
                                      (("--run-mode", "association_test", "--pval-method", "se"),
                                       "needs --pval-method loo"),
                                      (("--run-mode", "association_test"), "needs --pval-method loo")])
def test_cli_trait_file_needs_the_loo_association_test(traits, mode, why):
    _fatal(cli(*mode, "--trait-file", traits["good"]), "--trait-file", why)


def test_cli_trait_file_lines_are_checked(traits, files):
    d = traits["dir"]
    two = d / "two.txt"
    two.write_text("t0 %s %s\nt1 %s\n" % (files["phen"][0], d / "e_it_1.bin", files["phen"][1]))
    _fatal(cli(*LOO, "--trait-file", str(two)), "line 2", "2 fields")
    four = d / "four.txt"
    four.write_text("t0 %s %s extra\n" % (files["phen"][0], d / "e_it_1.bin"))
    _fatal(cli(*LOO, "--trait-file", str(four)), "line 1", "4 fields")
    dup = d / "dup.txt"
    dup.write_text("t0 %s %s\n# comment\nt0 %s %s\n" % (files["phen"][0], d / "e_it_1.bin", files["phen"][0],
                                                        d / "f_it_1.bin"))
    _fatal(cli(*LOO, "--trait-file", str(dup)), "line 3", "duplicate name", "t0")
    noit = d / "noit.txt"
    noit.write_text("t0 %s %s\n" % (files["phen"][0], d / "estimate.bin"))
    _fatal(cli(*LOO, "--trait-file", str(noit)), "cannot parse the iteration", "estimate.bin")
    _fatal(cli(*LOO, "--trait-file", str(d / "absent.txt")), "could not open trait file")


def test_cli_trait_file_rows_are_resolved_before_the_device(traits, files):
    _fatal(cli(*LOO, "--trait-file", traits["good"]), "NAN in data!", "y1.phen")
    bad = traits["dir"] / "swapped.txt"
    bad.write_text("a %s x_it_1.bin\nb %s y_it_1.bin\n" % (files["phen"][0], files["swapped"]))
    _fatal(cli(*LOO, "--trait-file", str(bad), "--phen-na", "drop"), "swapped.phen", "row 7")
    r = cli(*LOO, "--trait-file", traits["good"], "--phen-na", "drop", "--keep-file", files["keep"])
    assert "INFO   : kept 5 of 12 samples (5 not in the keep file, 2 with an NA phenotype)" in r.stdout
    assert "INFO   : NA phenotypes: t0 0 t1 1 t2 2" in r.stdout
