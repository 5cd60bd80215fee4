"""Writes tests/golden/tie_order.npz: what the compiled reference (oracle/_ref, built by build() where the reference's
sources are present) returns for the inputs of tests/tie_order_cases.py.

  <case>.rows    int32 [Nq, min(max_count, 128)]  batch_nanoflann_neighbors' matrix, cut to the library's widest row
  <case>.mc      int32                            its untruncated width
  random.digest  uint8 [300, 32]                  SHA-256 of every randomised cloud's matrix cut to its limit

    python scripts/gen_tie_order_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import tie_order_cases as tc  # noqa: E402
from oracle import native  # noqa: E402


def main():
    if not native.ref_available():
        raise SystemExit("oracle/_ref is not built: this script needs the reference's sources")
    out = {}
    for name in tc.NAMES:
        c = tc.cases()[name]
        rows = native.ref_radius_neighbors(c.qry, c.sup, c.q_lens, c.s_lens, c.radius)
        out[f"{name}.rows"] = rows[:, :128].astype(np.int32)
        out[f"{name}.mc"] = np.int32(rows.shape[1])
    digs = []
    for k in range(tc.N_RANDOM):
        c, limit = tc.random_case(k)
        rows = native.ref_radius_neighbors(c.qry, c.sup, c.q_lens, c.s_lens, c.radius)
        digs.append(tc.digest(rows[:, :limit]))
    out["random.digest"] = np.stack(digs)
    np.savez_compressed(tc.GOLDEN, **out)
    print(f"wrote {tc.GOLDEN}: {os.path.getsize(tc.GOLDEN)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
