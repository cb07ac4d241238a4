"""Regenerates tests/golden/spherical_basis_reference.npz.  Run ONLY in the build container:

    python -B tests/golden/make_dimenet_fixtures.py

Sources (data only; no reference source text is stored):

* ``spherical_basis_0`` (60 x 100) and a row subset of ``spherical_basis_1`` (954 x 100, rows ``rows_1``) of the
  reference's test asset ``test/assets/bessel_basis_reference.npz`` (loaded with ``allow_pickle=False``): the output of
  ``SphericalBasisLayer(10, 10, 5.0)`` on the two molecules of ``test/test_geom.py:17-60``, whose coordinates and edge
  lists are ``x0, x1, ei0, ei1`` of ``bessel_basis_reference.npz``.
* ``angles_0`` / ``angles_1``: the edge pairs of the reference's NumPy-only ``kgcnn.graph.adj.get_angle_indices``
  (imported from the reference tree with ``python -B``) for ``ei0`` / ``ei1``.
* ``zeros_L_R`` / ``norm_L_R`` for (7, 6) and (10, 10): the Bessel zeros and normalisation of
  kgcnn/ops/polynom.py:201-245, restated here with scipy (brentq on the same float32-rounded brackets, jv).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def bessel_tables(n, k):
    import scipy.special as sps
    from scipy.optimize import brentq

    def jn(r, order):
        return np.sqrt(np.pi / (2 * r)) * sps.jv(order + 0.5, r)

    zerosj = np.zeros((n, k), dtype="float32")
    zerosj[0] = np.arange(1, k + 1) * np.pi
    points = np.arange(1, k + n) * np.pi
    racines = np.zeros(k + n - 1, dtype="float32")
    for i in range(1, n):
        for j in range(k + n - 1 - i):
            racines[j] = brentq(jn, points[j], points[j + 1], (i,))
        points = racines
        zerosj[i][:k] = racines[:k]
    norm = np.array([1 / np.array([0.5 * jn(zerosj[o, i], o + 1) ** 2 for i in range(k)]) ** 0.5 for o in range(n)])
    return zerosj, norm.astype(np.float64)


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    from kgcnn.graph.adj import get_angle_indices
    src = np.load(os.path.join(REF, "test/assets/bessel_basis_reference.npz"), allow_pickle=False)
    geo = np.load(os.path.join(HERE, "bessel_basis_reference.npz"), allow_pickle=False)
    out = {"spherical_basis_0": src["spherical_basis_0"]}
    _, _, a0 = get_angle_indices(geo["ei0"])
    _, _, a1 = get_angle_indices(geo["ei1"])
    out["angles_0"], out["angles_1"] = np.asarray(a0, np.int64), np.asarray(a1, np.int64)
    rows = np.sort(np.random.default_rng(5).choice(len(a1), size=240, replace=False)).astype(np.int64)
    out["rows_1"], out["spherical_basis_1_rows"] = rows, src["spherical_basis_1"][rows]
    for n, k in ((7, 6), (10, 10)):
        z, nrm = bessel_tables(n, k)
        out["zeros_%d_%d" % (n, k)], out["norm_%d_%d" % (n, k)] = z, nrm
    np.savez_compressed(os.path.join(HERE, "spherical_basis_reference.npz"), **out)
    print("angle pairs:", len(a0), len(a1), "fixture bytes:",
          os.path.getsize(os.path.join(HERE, "spherical_basis_reference.npz")))


if __name__ == "__main__":
    main()
