#!/usr/bin/env python3
"""Records tests/golden/front_errors.json: the return code, the gsim_last_error() text and whether `*out` was cleared, for every case
of tests/front_errors_cases.py -- the argument and state errors of the two-table fronts and gsim_db_knn on tables that are not on a
GPU.  Needs no GPU.  Run it on a build of the commit whose behaviour is to be kept (GSIM_LIB names another build of the library),
never on the code under test: tests/test_front_errors_host.py replays the list and demands equality.

  GSIM_LIB=/path/to/parent/libgsim_hip.so python scripts/make_front_errors_golden.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from front_errors_cases import run_all  # noqa: E402

if __name__ == "__main__":
    got = run_all()
    path = os.path.join(ROOT, "tests", "golden", "front_errors.json")
    with open(path, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True, allow_nan=False)
        f.write("\n")
    print("%d cases -> %s" % (len(got), path))
