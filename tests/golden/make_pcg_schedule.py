"""Records tests/golden/pcg_schedule.json, the fixture of
tests/test_gpu_pcg_schedule.py, on a GPU:

    python tests/golden/make_pcg_schedule.py [OUT.json]

Every case runs twice; a field that differs between the two runs is left out
of the fixture and reported.  Run it on the commit whose schedule is to be
pinned (the parent of a change to pcg.cpp), never on the change itself."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import pytest  # noqa: E402

import test_gpu_pcg_schedule as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    fixture, unstable = {}, []
    for name in sorted(T.CASES):
        runs = []
        for _ in range(2):
            with pytest.MonkeyPatch.context() as mp:
                runs.append(T.run_case(name, mp))
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
