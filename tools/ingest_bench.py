"""Streaming ingest rate (vampomi_load_meth_file): write a marker-major fp64
file of the given shape (generated on the device, dumped in chunks), then
time loading it into a fresh context (parallel pread -> pinned staging ->
HBM, plus the marker statistics), and check it bit for bit.

    python tools/ingest_bench.py [--adjust C] [--dtype f32] [--keep] [N] [M] [path] [threads...]

--adjust C: the timed loads regress C random covariates and the intercept out
of every marker (Data(adjust=Z): staging -> fp64 work block -> vk::adjust_cols);
the check is then that two markers hold the bits that a two-marker context
holds after loading them from the host (neither the chunk nor the route
matters), and that they are orthogonal to the basis.  --keep: use the file at
`path` if it is there, and leave it there (several runs over one file).
--dtype f32: the file holds the values rounded to floats and is loaded into the
default fp64 storage (staging -> vk::convert_cols); GB/s counts the file's bytes.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import vampomi_amd as va  # noqa: E402

argv = sys.argv[1:]
adjust_C = None
if "--adjust" in argv:
    i = argv.index("--adjust")
    adjust_C = int(argv[i + 1])
    del argv[i:i + 2]
dtype = "f64"
if "--dtype" in argv:
    i = argv.index("--dtype")
    dtype = argv[i + 1]
    del argv[i:i + 2]
es, ftype = {"f64": (8, "<f8"), "f32": (4, "<f4")}[dtype]
keep = "--keep" in argv
if keep:
    argv.remove("--keep")
N = int(argv[0]) if len(argv) > 0 else 100000
M = int(argv[1]) if len(argv) > 1 else 25000
path = argv[2] if len(argv) > 2 else os.path.join(os.environ.get("TMPDIR", "/tmp"), "vampomi_ingest.bin")
threads = argv[3:] or ["1", "4", "8", "16"]
gb = float(es) * N * M / 1e9
t0 = time.perf_counter()
with va.Data(N, M) as d:
    d.generate(5, va.GEN_METH)
    ref_rows = d.get_meth_data(M // 2, 2)
    ref_mave = d.get_mave()
    if not (keep and os.path.exists(path) and os.path.getsize(path) == es * N * M):
        with open(path, "wb") as f:
            step = max(1, (1 << 30) // (8 * N))
            for i0 in range(0, M, step):
                f.write(d.get_meth_data(i0, min(step, M - i0)).astype(ftype).tobytes())
t_write = time.perf_counter() - t0
ref_rows = ref_rows.astype(ftype).astype(np.float64)  # what the file holds, widened
kw = {}
if adjust_C is not None:
    Z = np.random.default_rng(7).uniform(-1.0, 1.0, (N, adjust_C))
    kw = {"adjust": Z}
    t0 = time.perf_counter()
    with va.Data(N, 2, **kw) as d:
        basis_s = time.perf_counter() - t0  # (opening the context: the host's Gram-Schmidt is in it)
        d.load_meth(ref_rows)
        ref_rows = d.get_meth_data()
        Q = d.adjust_info()["Q"]
res = {"N": N, "M": M, "GB": round(gb, 2), "write_s": round(t_write, 1), "adjust": adjust_C, "dtype": dtype, "runs": []}
if adjust_C is not None:
    res["basis_s"] = round(basis_s, 3)
for nt in threads:
    os.environ["VAMPOMI_IO_THREADS"] = nt
    with va.Data(N, M, **kw) as d:
        t0 = time.perf_counter()
        d.read_methylation_data(path, dtype)
        el = time.perf_counter() - t0
        rows = d.get_meth_data(M // 2, 2)
        ok = bool(np.array_equal(rows, ref_rows))
        if adjust_C is None and dtype == "f64":
            ok = ok and bool(np.array_equal(d.get_mave(), ref_mave))
        elif adjust_C is not None:
            ok = ok and bool(np.abs(rows @ Q).max() <= 1e-11)
    res["runs"].append({"threads": int(nt), "s": round(el, 3), "GB/s": round(gb / el, 2), "bitwise": ok})
    print(json.dumps(res["runs"][-1]), flush=True)
if not keep:
    os.remove(path)
print(json.dumps(res))
