"""Records tests/golden/vamp_step_schedule.json, the fixture of
tests/test_gpu_vamp_schedule.py, on a GPU:

    python tests/golden/make_vamp_step_schedule.py [OUT.json]

Every case runs twice; a field that differs between the two runs is left out
of the fixture and reported.  Run it on the commit whose schedule is to be
pinned (the parent of a change to the iteration in vamp.cpp), never on the
change itself.

    python tests/golden/make_vamp_step_schedule.py --nmse

prints, for the early-stop cases run to max_iter with the stop off, the
stopping rule's NMSE = ||x1_prev - x1|| / ||x1_prev|| per iteration (from the
x1 history), from which their stop_criteria_thr is chosen."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import numpy as np  # noqa: E402
import pytest  # noqa: E402

import test_gpu_pcg_schedule as P  # noqa: E402
import test_gpu_vamp_schedule as T  # noqa: E402


def nmse_traces():
    for name, case in sorted(T.CASES.items()):
        if not case.get("step_after_stop"):
            continue
        case = dict(case, opts=dict(case["opts"], stop_criteria_thr=0.0), step_after_stop=False)
        with P.va.Data(case["N"], case["Mt"]) as d:
            _, x1, _ = P._run_vamp(d, case)
        nmse = [float(np.linalg.norm(x1[k - 1] - x1[k]) / np.linalg.norm(x1[k - 1])) for k in range(1, len(x1))]
        print(name, "NMSE at iterations 2..:", json.dumps(nmse), flush=True)


def main():
    if "--nmse" in sys.argv:
        return nmse_traces()
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    fixture, unstable = {}, []
    for name in sorted(T.CASES):
        runs = []
        for _ in range(2):
            with pytest.MonkeyPatch.context() as mp:
                runs.append(P.run_case(name, mp, T.CASES))
        fixture[name] = {k: v for k, v in runs[0].items() if runs[1].get(k) == v}
        unstable += [(name, k, runs[0][k], runs[1].get(k)) for k in runs[0] if runs[1].get(k) != runs[0][k]]
        print(name, json.dumps(fixture[name]), flush=True)
    for u in unstable:
        print("differs between two runs, left out:", u)
    with open(out, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "unstable fields:", len(unstable))


if __name__ == "__main__":
    main()
