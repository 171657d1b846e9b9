"""Records which launches every case of tests/search_routes_spec.py takes -> tests/golden/search_routes.json.

Run it on the commit whose routing is the reference (a refactor of the search front end: its parent); tests/test_zz_gpu_search_routes.py
then holds later commits to the same `count:<stage>` deltas.  Every group runs in a child process (the switches are read once per process).

    python scripts/record_search_routes.py [output.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import search_routes_spec as spec      # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else spec.GOLDEN
    table = {"default": spec.run_in_child({}, list(spec.CASES))}
    print("default", flush=True)
    for group, (env, names) in spec.SWITCHED.items():
        table[group] = spec.run_in_child(env, names)
        print(group, flush=True)
    with open(out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
