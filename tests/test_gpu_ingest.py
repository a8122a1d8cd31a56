"""Streaming ingest (read_methylation_data, src/data.cpp:116-153 +
compute_markers_statistics :233-283): a marker-major fp64 file larger than
the 256 MB staging buffers, with ragged N, read by several threads, lands in
HBM bit for bit; the statistics match the oracle."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")
from oracle import pyoracle as O  # noqa: E402  (checker)


@pytest.mark.parametrize("threads", ["1", "5"])
def test_multichunk_file_ingest(tmp_path, monkeypatch, threads):
    monkeypatch.setenv("VAMPOMI_IO_THREADS", threads)
    N, Mt = 4099, 20011  # 656 MB: three staging chunks, the last one partial
    X = O.generate_markers(31, 1, N, 0, Mt)
    p = tmp_path / "big.bin"
    X.tofile(p)
    with va.Data(N, Mt) as d:
        d.read_methylation_data(str(p))
        for i0 in (0, 8180, 8181, 16362, Mt - 3):
            assert np.array_equal(d.get_meth_data(i0, 3), X[i0:i0 + 3])
        mo, so = O.marker_stats(X)
        assert relerr(d.get_mave(), mo) < 1e-13 and relerr(d.get_msig(), so) < 1e-13


@pytest.fixture(scope="module")
def second_trip():
    """A float32 chunk of 4100 x 4099 = 16 805 900 elements, past the 65536 x 256
    threads of the conversion kernels' grid: its last 28 684 elements are
    converted on the grid-stride loop's second trip.  In that tail, a 1.0
    (stored as 65535, clamped) and, as the very last element, an exact tie
    (k + 0.5) * 2^-16 with k even, which rounds down to k.  Returns (X, what
    numpy's rint stores, the clamps, the largest error), made once."""
    N, M, k = 4099, 4100, 40000
    X = np.random.default_rng(20).random((M, N), dtype=np.float32)
    first = 65536 * 256  # the second trip's first element
    assert first < M * N - 1 < 2 * first
    X.reshape(-1)[first + 1000] = 1.0
    X.reshape(-1)[-1] = (k + 0.5) / 65536
    x = X.astype(np.float64)
    r = np.rint(x * 65536)
    assert x[-1, -1] * 65536 == k + 0.5 and r[-1, -1] == k and r.reshape(-1)[first + 1000] == 65536
    want = np.minimum(65535, r) * 2.0**-16
    return X, want, int(np.count_nonzero(r > 65535)), float(np.abs(want - x).max())


@pytest.mark.parametrize("subset", [False, True], ids=["all_rows", "row_subset"])
def test_u16_conversion_on_the_second_grid_stride_trip(second_trip, subset):
    X, want, clamped, max_err = second_trip
    M, N = X.shape
    if subset:  # 4099 of 4200 file rows; what a dropped row holds (out of range) is neither stored nor counted
        N_file = 4200
        rows = np.sort(np.random.default_rng(21).choice(N_file, N, replace=False))
        Xin = np.full((M, N_file), 2.0, dtype=np.float32)
        Xin[:, rows] = X
        d = va.Data(N_file, M, storage="u16", rows=rows)
    else:
        Xin, d = X, va.Data(N, M, storage="u16")
    with d:
        d.load_meth(Xin)
        got, qs = d.get_meth_data(), d.quant_stats()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert qs["clamped"] == clamped >= 1 and qs["max_abs_err"] == max_err


def test_short_file_is_an_error(tmp_path):
    N, Mt = 100, 50
    p = tmp_path / "short.bin"
    np.zeros((Mt - 1) * N).tofile(p)
    with va.Data(N, Mt) as d:
        with pytest.raises(va.VampomiError) as e:
            d.read_methylation_data(str(p))
        assert e.value.status == 4
