"""The bit pin of the association tests: SHA-256 digests of the statistics and
p-values that assoc_loo, assoc_loo_multi and assoc_loco return on small fixed
problems, on one GPU.

    python tools/assoc_pin.py            compare this build with tests/golden/assoc_bits_pin.json
    python tools/assoc_pin.py --write    record the file (names and hex strings only)

Record with the library the pin is to stand for, chosen through VAMPOMI_LIB
(tools/gpu_session.sh), BEFORE a change to the kernels; tests/test_gpu_assoc_pin.py
then holds every later build to it.  The cases and the digests are made here
for both, so the test and the record cannot drift apart.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
import numpy as np  # noqa: E402

PIN = os.path.join(ROOT, "tests", "golden", "assoc_bits_pin.json")
# (N, Mt, generator kind) of tests/test_gpu_assoc_multi.py: odd N with the pad
# row, several load rounds and an unrolled round; fewer markers than a
# workgroup's G; N below one load round (the tail loop alone)
SHAPES = [(4099, 301, 1), (257, 5, 1), (5, 7, 0)]
CASES = [(s, st) for st in ("f64", "f32", "u16") for s in SHAPES if st != "u16" or s[2] == 1]
LOO_VARIANTS = (16, 0)  # the default workgroup kernel; the wave-per-marker loo_kernel<4, 2, true>
MULTI_T = (2, 3, 4, 5)  # KT = 2, 3, 4 and a chunk of four with a remainder of one
LOCO_LABELS = "g5"      # tests/_assoc_loco.py: 5 labels, one unused, one of a single marker


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


def digests():
    """{name: hex digest} of every case on the library vampomi_amd loads."""
    import _assoc_loco as L
    import _assoc_multi as H
    import vampomi_amd as va

    out = {}

    def put(name, p, s):
        out[name + "/pvals"] = _sha(p)
        out[name + "/stats"] = _sha(s)

    for (N, Mt, kind), storage in CASES:
        X, Y, est = H.problem(N, Mt, kind, T=max(MULTI_T))
        lab, G = L.labels(LOCO_LABELS, Mt)
        case = "%dx%d_kind%d/%s" % (N, Mt, kind, storage)
        with va.Data(N, Mt, storage=storage) as d:
            d.load_meth(X)
            d.set_phen(Y[0], standardize=False)
            for v in LOO_VARIANTS:
                d.set_variant(2, v)
                put("%s/loo_v%d" % (case, v), *d.assoc_loo(est[0]))
            d.set_variant(2, 16)  # the default
            for T in MULTI_T:
                put("%s/multi_T%d" % (case, T), *d.assoc_loo_multi(Y[:T], est[:T], standardize=False))
            put("%s/loco_est" % case, *d.assoc_loco(est[0], lab, G=G))
            put("%s/loco_noest" % case, *d.assoc_loco(None, lab, G=G))
    return out


def recorded():
    with open(PIN) as f:
        return json.load(f)


if __name__ == "__main__":
    got = digests()
    if "--write" in sys.argv[1:]:
        with open(PIN, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote %d digests to %s" % (len(got), os.path.relpath(PIN, ROOT)))
    else:
        ref = recorded()
        bad = sorted(k for k in set(got) | set(ref) if got.get(k) != ref.get(k))
        print("%d of %d digests differ" % (len(bad), len(ref)), *bad[:20], sep="\n")
        sys.exit(1 if bad else 0)
