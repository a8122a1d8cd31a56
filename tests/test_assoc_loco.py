"""The leave-one-chromosome-out test without a device: the
ABI additions (vampomi_assoc_loco, vampomi_read_labels), the label file, and
the checks of --pval-method loco / --loco-file, which all end on the host
before the context is opened.  (Before the method existed, --pval-method loco
wrote no file and exited 0.)"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import vampomi_amd as va
from vampomi_amd import _lib


def test_symbols_and_abi_version():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("vampomi_assoc_loco", "vampomi_read_labels"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert va.load().vampomi_abi_version() == 3
    assert C.sizeof(_lib.Stats) == 17 * 48 + 16  # vampomi_stats keeps its layout
    assert hasattr(va.Data, "assoc_loco") and "read_labels" in va.__all__


def test_labels_are_numbered_by_first_appearance(tmp_path):
    p = tmp_path / "lab.txt"
    p.write_text("chr7 X\t1 chr7\n\n\n  1\t\tX\r\nchr10 1 chr7   \n\n")
    lab, names = va.read_labels(str(p), 9)  # tabs, blank lines, a carriage return, trailing blanks
    assert lab.dtype == np.int32 and lab.tolist() == [0, 1, 2, 0, 2, 1, 3, 2, 0]
    assert names == ["chr7", "X", "1", "chr10"]


def test_one_token_per_line_and_one_line(tmp_path):
    toks = ["b", "a", "b", "c", "a", "a", "10", "9", "10", "b"]
    want = [0, 1, 0, 2, 1, 1, 3, 4, 3, 0]
    for sep in ("\n", " ", "\t", "\n\n", " \t\n"):
        p = tmp_path / "lab.txt"
        p.write_text(sep.join(toks) + ("\n" if sep != " " else ""))
        lab, names = va.read_labels(str(p), len(toks))
        assert lab.tolist() == want and names == ["b", "a", "c", "10", "9"], repr(sep)


def test_a_wrong_token_count(tmp_path):
    p = tmp_path / "lab.txt"
    p.write_text("1 1 2 2 3\n")
    for Mt in (4, 6):
        with pytest.raises(va.VampomiError) as e:
            va.read_labels(str(p), Mt)
        assert e.value.status == 1 and "5 labels" in str(e.value) and "expected %d" % Mt in str(e.value)
    assert va.read_labels(str(p), 5)[0].tolist() == [0, 0, 1, 1, 2]
    with pytest.raises(va.VampomiError) as e:
        va.read_labels(str(tmp_path / "absent.txt"), 5)
    assert e.value.status == 4


def test_sixty_four_labels_pass_and_sixty_five_do_not(tmp_path):
    p = tmp_path / "lab.txt"
    p.write_text(" ".join("c%d" % (i % 64) for i in range(200)))
    lab, names = va.read_labels(str(p), 200)
    assert lab.tolist() == [i % 64 for i in range(200)] and names == ["c%d" % i for i in range(64)]
    p.write_text(" ".join("c%d" % (i % 65) for i in range(200)))
    with pytest.raises(va.VampomiError) as e:
        va.read_labels(str(p), 200)
    assert e.value.status == 1 and "more than 64 distinct labels" in str(e.value) and "'c64'" in str(e.value)


def test_the_c_call_counts_and_checks_the_names_buffer(tmp_path):
    lib = va.load()
    p = tmp_path / "lab.txt"
    p.write_text("x y x\n")
    G = C.c_int(-1)
    assert lib.vampomi_read_labels(str(p).encode(), 3, None, C.byref(G), None, 0) == 0 and G.value == 2
    buf = C.create_string_buffer(4)
    assert lib.vampomi_read_labels(str(p).encode(), 3, None, None, buf, 4) == 1  # "x\ny\n" and the NUL need 5
    buf = C.create_string_buffer(5)
    assert lib.vampomi_read_labels(str(p).encode(), 3, None, None, buf, 5) == 0 and buf.value == b"x\ny\n"
    assert lib.vampomi_read_labels(None, 3, None, None, None, 0) == 1


# ---- CLI: all of these end before the device is opened ----
def cli(*args, Mt=20):
    return subprocess.run([va.CLI_PATH, "--meth-file", "absent.bin", "--N", "12", "--Mt", str(Mt), "--out-dir", ".",
                           "--phen-file", "absent.phen", *args], capture_output=True, text=True, timeout=120)


LOCO = ("--run-mode", "association_test", "--pval-method", "loco", "--estimate-file", "e_it_3.bin")


def _fatal(r, *words):
    assert r.returncode == 1, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("FATAL")]
    assert len(lines) == 1 and all(w in lines[0] for w in words), r.stdout
    assert "cannot open the device context" not in r.stdout


@pytest.fixture(scope="module")
def labels(tmp_path_factory):
    d = tmp_path_factory.mktemp("loco")
    good = d / "good.txt"
    good.write_text("\n".join(["1"] * 7 + ["X"] * 6 + ["chr2"] * 7) + "\n")
    return {"dir": d, "good": str(good)}


def test_cli_loco_needs_its_label_file():
    _fatal(cli(*LOCO), "--pval-method loco", "needs --loco-file")


@pytest.mark.parametrize("mode,why", [(("--run-mode", "infere", "--pval-method", "loco"),
                                       "needs --run-mode association_test"),
                                      (("--run-mode", "test", "--pval-method", "loco"),
                                       "needs --run-mode association_test"),
                                      (("--run-mode", "association_test", "--pval-method", "loo"),
                                       "needs --pval-method loco"),
                                      (("--run-mode", "association_test", "--pval-method", "se"),
                                       "needs --pval-method loco"),
                                      (("--run-mode", "association_test"), "needs --pval-method loco")])
def test_cli_loco_file_needs_the_loco_association_test(labels, mode, why):
    _fatal(cli(*mode, "--loco-file", labels["good"]), "--loco-file", why)


def test_cli_loco_file_cannot_stand_beside_a_trait_file(labels):
    r = subprocess.run([va.CLI_PATH, "--meth-file", "absent.bin", "--N", "12", "--Mt", "20", "--out-dir", ".",
                        "--run-mode", "association_test", "--pval-method", "loco", "--loco-file", labels["good"],
                        "--trait-file", "traits.txt"], capture_output=True, text=True, timeout=120)
    _fatal(r, "--loco-file", "--trait-file")


def test_cli_label_file_is_checked_before_the_device(labels):
    _fatal(cli(*LOCO, "--loco-file", labels["good"], Mt=21), "--loco-file", "20 labels", "expected 21")
    _fatal(cli(*LOCO, "--loco-file", labels["good"], Mt=19), "--loco-file", "20 labels", "expected 19")
    many = labels["dir"] / "many.txt"
    many.write_text(" ".join(str(i) for i in range(65)))
    _fatal(cli(*LOCO, "--loco-file", str(many), Mt=65), "--loco-file", "more than 64 distinct labels")
    _fatal(cli(*LOCO, "--loco-file", str(labels["dir"] / "absent.txt")), "--loco-file", "cannot open")


def test_cli_prints_the_segments_and_goes_on(labels):
    """A good label file passes the host checks: rank 0 prints the segments, and
    the run ends only where it needs the phenotype file (or the device)."""
    r = cli(*LOCO, "--loco-file", labels["good"])
    assert "INFO   : LOCO: 3 segments (1:7 X:6 chr2:7)" in r.stdout
    assert r.returncode == 1  # absent.phen / no device


def test_cli_another_unknown_method_keeps_its_behaviour():
    """Any other unknown --pval-method still passes the option checks (the
    reference computes nothing for it)."""
    r = cli("--run-mode", "association_test", "--pval-method", "jackknife")
    assert "pval-method" not in "".join(ln for ln in r.stdout.splitlines() if ln.startswith("FATAL"))


# ---- the oracle alone: the label sets of the GPU tests give a different test ----
@pytest.mark.parametrize("shape", [(301, 257, 0), (1001, 517, 1)])
def test_the_oracle_shows_a_test_of_its_own(shape):
    """With the G = 5 label set the leave-one-chromosome-out p-values (the
    oracle's assoc_loo with the estimate zeroed inside the marker's label) are
    neither assoc_loo(est)'s nor the marginal test's: some marker differs by
    more than 1e-3 relative from each, and y - A (x1 zeroed inside c) agrees
    with (y - z) + z_c far inside the residual bar."""
    import _assoc_loco as L
    from oracle import pyoracle as O

    N, Mt, kind = shape
    X, y, est = L.problem(N, Mt, kind)
    lab, G = L.labels("g5", Mt)
    assert np.sum(lab == 2) == 0 and np.sum(lab == 1) == 1 and np.all(lab[:7] == 0)
    assert np.any(np.diff(np.flatnonzero(lab == 3)) > 1)  # not contiguous
    ref = L.oracle_refs(X, y, est, lab, G)
    assert L.differs(ref["p"], O.assoc_loo(X, y, est)[0])
    assert L.differs(ref["p"], O.assoc_loo(X, y, np.zeros(Mt))[0])
    mave, msig = O.marker_stats(X)
    x1 = est * np.sqrt(N)
    zc = [O.ax(X, mave, msig, np.where(lab == c, x1, 0.0)) for c in range(G)]
    z = zc[0].copy()
    for c in range(1, G):
        z = z + zc[c]
    L.check_resid(np.stack([(y - z) + zc[c] for c in range(G)]), ref["R"], ref["scale"], "identity")
