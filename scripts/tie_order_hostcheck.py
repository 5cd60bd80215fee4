"""Compiles scripts/tie_order_hostcheck.cpp -- csrc/tie_order.h plus a small main, no HIP, nothing loaded into Python --
with -fsanitize=address,undefined and runs it over the case list of tests/tie_order_cases.py (every case at every
limit, and the 300 randomised clouds), expecting the reference's rows from tests/golden/tie_order.npz where they are
stored.  CPU only.

    python scripts/tie_order_hostcheck.py [--cxx g++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import tie_order_cases as tc  # noqa: E402


def record(c, rows, mc, want):
    nb = len(c.s_lens)
    cu = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    parts = [np.array([len(c.qry), len(c.sup), nb, rows.shape[1], mc], np.int32), np.array([c.radius], np.float32),
             cu(c.q_lens), cu(c.s_lens), c.qry.astype(np.float32), c.sup.astype(np.float32), rows.astype(np.int32),
             want.astype(np.int32)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="g++")
    args = ap.parse_args()
    gold = tc.load_golden()
    blob = []
    for name in tc.NAMES:
        for limit in tc.LIMITS:
            rows, mc = tc.index_rows(name, limit)
            blob.append(record(tc.cases()[name], rows, mc, tc.reference_rows(gold, name, limit)))
    from oracle import native
    if native.ref_available():
        for k in range(tc.N_RANDOM):
            c, limit = tc.random_case(k)
            rows, mc = tc.index_rows(c.name, limit)
            want = native.ref_radius_neighbors(c.qry, c.sup, c.q_lens, c.s_lens, c.radius)[:, :limit]
            blob.append(record(c, rows, mc, want))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tie_order_hostcheck")
        subprocess.run([args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(REPO, "scripts", "tie_order_hostcheck.cpp")],
                       check=True)
        r = subprocess.run([exe], input=b"".join(blob))
    print(f"{len(blob)} records, exit status {r.returncode}")
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
