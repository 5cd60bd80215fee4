"""Writes tests/golden/subsample_attrs.npz: what the reference's batch_grid_subsampling returns for the inputs of
tests/subsample_attrs_cases.py (the cases of REFERENCE_DEFINED; the inputs regenerate from their seeds).

  <case>.lens   int32 [nb]         subsampled lengths
  <case>.pts    float32 [M, 3]     barycentres, in the reference's row order
  <case>.feat   float32 [M, fdim]  averaged features (cases with features)
  <case>.lab    int32 [M, ldim]    voted labels (cases with labels)

The reference's grid_subsampling.cpp and cloud.cpp are compiled where they lie, with the flags of its setup.py
(-std=c++11 -D_GLIBCXX_USE_CXX11_ABI=0, default x86-64 code generation: no FMA contraction) and the small driver below,
into a temporary directory that is removed afterwards.

    python scripts/gen_subsample_attrs_golden.py /path/to/reference
"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import subsample_attrs_cases as sc  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "subsample_attrs.npz")
WRAPPERS = os.path.join("src", "models", "backbone_kpconv", "cpp_wrappers")

DRIVER = r"""
#include <cstring>
#include "grid_subsampling/grid_subsampling.h"

extern "C" long attrs_subsample_batch(const float* pts, int n, const int* lens, int nb, float dl, int max_p,
                                      const float* feat, int fdim, const int* lab, int ldim, float* out_pts,
                                      float* out_feat, int* out_lab, int* out_lens) {
  std::vector<PointXYZ> points((const PointXYZ*)pts, (const PointXYZ*)pts + n), sub_points;
  std::vector<float> features, sub_features;
  std::vector<int> classes, sub_classes, batches(lens, lens + nb), sub_batches;
  if (fdim > 0) features.assign(feat, feat + (size_t)n * fdim);
  if (ldim > 0) classes.assign(lab, lab + (size_t)n * ldim);
  batch_grid_subsampling(points, sub_points, features, sub_features, classes, sub_classes, batches, sub_batches, dl,
                         max_p);
  std::memcpy(out_pts, sub_points.data(), sub_points.size() * sizeof(PointXYZ));
  std::memcpy(out_feat, sub_features.data(), sub_features.size() * sizeof(float));
  std::memcpy(out_lab, sub_classes.data(), sub_classes.size() * sizeof(int));
  std::memcpy(out_lens, sub_batches.data(), sub_batches.size() * sizeof(int));
  return (long)sub_points.size();
}
"""


def build(ref_root, tmp):
    cpp = os.path.join(ref_root, WRAPPERS)
    srcs = [os.path.join(cpp, "cpp_subsampling", "grid_subsampling", "grid_subsampling.cpp"),
            os.path.join(cpp, "cpp_utils", "cloud", "cloud.cpp")]
    for s in srcs:
        if not os.path.exists(s):
            raise SystemExit(f"{s} is missing: pass the root of the reference tree")
    driver, lib = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "libattrs_ref.so")
    with open(driver, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++11", "-D_GLIBCXX_USE_CXX11_ABI=0", "-O2", "-fPIC", "-shared",
                           "-I" + os.path.join(cpp, "cpp_subsampling"), "-o", lib, driver] + srcs)
    fn = ctypes.CDLL(lib).attrs_subsample_batch
    fn.restype = ctypes.c_long
    vp, i = ctypes.c_void_p, ctypes.c_int
    fn.argtypes = [vp, i, vp, i, ctypes.c_float, i, vp, i, vp, i, vp, vp, vp, vp]
    return fn


def run(fn, c):
    n, nb, fdim, ldim = len(c.pts), len(c.lens), sc.fdim(c), sc.ldim(c)
    lens = np.asarray(c.lens, np.int32)
    out_pts, out_lens = np.empty((n, 3), np.float32), np.empty(nb, np.int32)
    out_feat, out_lab = np.empty((n, fdim), np.float32), np.empty((n, ldim), np.int32)
    p = lambda a: None if a is None else a.ctypes.data
    m = fn(p(c.pts), n, p(lens), nb, c.dl, c.max_p, p(c.feat), fdim, p(c.lab), ldim, p(out_pts), p(out_feat),
           p(out_lab), p(out_lens))
    assert m == int(out_lens.sum())
    return out_pts[:m].copy(), out_lens, out_feat[:m].copy(), out_lab[:m].copy()


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    tmp = tempfile.mkdtemp(prefix="subsample_attrs_ref_")
    try:
        fn = build(sys.argv[1], tmp)
        out = {}
        for name in sc.REFERENCE_DEFINED:
            c = sc.cases()[name]
            pts, lens, feat, lab = run(fn, c)
            out[f"{name}.lens"], out[f"{name}.pts"] = lens, pts
            if sc.fdim(c):
                out[f"{name}.feat"] = feat
            if sc.ldim(c):
                out[f"{name}.lab"] = lab
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
