#!/usr/bin/env python3
"""Records a golden file of front errors: the return code, the gsim_last_error() text and what became of the outputs, for every case
of a case list -- the argument and state errors of the fronts on tables that are not on a GPU.  Needs no GPU.  Five lists:

  two-table  tests/front_errors_cases.py -> tests/golden/front_errors.json (the two-table fronts and gsim_db_knn;
             replayed by tests/test_front_errors_host.py)
  single     tests/single_front_errors_cases.py -> tests/golden/single_front_errors.json (the single-table fronts and the host
             functions on a caller's CSR graph; replayed by tests/test_single_front_errors_host.py)
  cluster    tests/cluster_front_errors_cases.py -> tests/golden/cluster_front_errors.json (the clustering fronts that came
             later and their host functions; replayed by tests/test_cluster_front_errors_host.py)
  popindex   tests/popindex_front_errors_cases.py -> tests/golden/popindex_front_errors.json (the popcount-index calls; replayed by
             tests/test_popindex_host.py)
  rowhash    tests/rowhash_front_errors_cases.py -> tests/golden/rowhash_front_errors.json (the row-hash calls; replayed by
             tests/test_rowhash_host.py)

Run it on a build of the commit whose behaviour is to be kept (GSIM_LIB names another build of the library), never on the code
under test: the tests replay the list and demand equality.

  GSIM_LIB=/path/to/parent/libgsim_hip.so python scripts/make_front_errors_golden.py [two-table|single|cluster|popindex|rowhash]"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

LISTS = {"two-table": ("front_errors_cases", "front_errors.json"), "single": ("single_front_errors_cases", "single_front_errors.json"),
         "cluster": ("cluster_front_errors_cases", "cluster_front_errors.json"),
         "popindex": ("popindex_front_errors_cases", "popindex_front_errors.json"),
         "rowhash": ("rowhash_front_errors_cases", "rowhash_front_errors.json")}

if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "two-table"
    if which not in LISTS:
        sys.exit("usage: make_front_errors_golden.py [%s]" % "|".join(LISTS))
    module, name = LISTS[which]
    got = importlib.import_module(module).run_all()
    path = os.path.join(ROOT, "tests", "golden", name)
    with open(path, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True, allow_nan=False)
        f.write("\n")
    print("%d cases -> %s" % (len(got), path))
