"""Regenerates tests/golden/periodic_cases.npz.  Run ONLY in the build container:

    python -B tests/golden/make_periodic_fixtures.py

Source (data only; no reference source text is stored): the indices, images and distances that the reference's
NumPy-only ``kgcnn.graph.geom.range_neighbour_lattice`` (imported from the reference tree with ``python -B``) returns
with ``exclusive=True, self_loops=False`` for small periodic structures.  Coordinates and lattices are drawn from
``np.random.default_rng(103)`` in the order below, rounded to float32 (what the engine receives) and handed to the
reference as float64:

* ``cubic1``: ``L = 3.1 I``, one atom ``uniform(0, 3.1)``; cutoff 4 (six self-image edges).
* ``tri5``: ``L = [[3.0, 0.2, 0.1], [0.9, 2.8, -0.3], [0.4, 0.7, 3.3]]``, five atoms ``uniform(0, 1) @ L``; cutoffs 4.0
  (degrees below one wave of hits), 4.6 (degrees cross 64), 5.5 (degrees cross 128), and 4.0 with ``max_neighbours=12``.
* ``unwrapped``: ``tri5`` with atom 2 moved by ``2 a0 - a1``; cutoff 4 (the same number of edges, larger images).
* ``thin2``: two atoms ``uniform(0, 1) @ L`` in ``[[1.9, 0, 0], [0.3, 2.1, 0], [0, 0.2, 7.0]]``; cutoff 4 (a pair is
  connected through several images).
* ``big6``: six atoms ``uniform(0, 1) @ L`` in ``diag(11, 12, 13)``; cutoff 4 (atoms without neighbours).

The script asserts what the tests assume, so that the reference alone satisfies it: no distance lies within 1e-3 of its
cutoff; per receiver, distinct consecutive distances differ by more than 1e-5 (smaller gaps must be exact ties up to
1e-9); no ``max_neighbours`` cut falls inside a tie (the distances on both sides of the cut differ by more than 1e-5).
If a draw violates one, change the seed and write the new seed here.  Seeds tried: 100 (``tri5`` at 5.5 has two distinct
distances 5.5e-6 apart), 101 (passes, but no degree of ``tri5`` at 5.5 exceeds 128), 102 (a distance within 1e-3 of the
cutoff 4.0); 103 is the first that satisfies the three conditions and the degree ranges, which the script asserts too:
``tri5`` below 64 at 4.0, above 64 and below 128 at 4.6, some above 128 at 5.5; ``big6`` has an atom without
neighbours; the 12th and 13th distances of every ``tri5`` receiver differ by at least 2e-3.

Keys per case ``<c>``: ``xyz_<c>`` (N, 3) float32, ``lattice_<c>`` (3, 3) float32, ``cutoff_<c>`` float64,
``maxn_<c>`` int64 (-1: none), ``indices_<c>`` (M, 2) int64, ``images_<c>`` (M, 3) int64, ``dist_<c>`` (M,) float64;
``names`` lists the cases in order.

It also prints the reference's time for the 128 structures of ``gcnn_keras_amd.synth.periodic_structures`` at cutoffs
4 and 5 on this container's CPU (the yardstick quoted in DESIGN.md; the reference does not exist on the GPU machine).
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SEED = 103


def structures():
    rng = np.random.default_rng(SEED)
    tri = np.array([[3.0, 0.2, 0.1], [0.9, 2.8, -0.3], [0.4, 0.7, 3.3]])
    thin = np.array([[1.9, 0.0, 0.0], [0.3, 2.1, 0.0], [0.0, 0.2, 7.0]])
    big = np.diag([11.0, 12.0, 13.0])
    out = {}
    out["cubic1"] = (rng.uniform(0.0, 3.1, size=(1, 3)), 3.1 * np.eye(3))
    out["tri5"] = (rng.uniform(0.0, 1.0, size=(5, 3)) @ tri, tri)
    moved = out["tri5"][0].copy()
    moved[2] += 2.0 * tri[0] - tri[1]
    out["unwrapped"] = (moved, tri)
    out["thin2"] = (rng.uniform(0.0, 1.0, size=(2, 3)) @ thin, thin)
    out["big6"] = (rng.uniform(0.0, 1.0, size=(6, 3)) @ big, big)
    return {k: (x.astype(np.float32), lat.astype(np.float32)) for k, (x, lat) in out.items()}


CASES = [("cubic1_c40", "cubic1", 4.0, None), ("tri5_c40", "tri5", 4.0, None), ("tri5_c46", "tri5", 4.6, None),
         ("tri5_c55", "tri5", 5.5, None), ("tri5_c40_n12", "tri5", 4.0, 12), ("unwrapped_c40", "unwrapped", 4.0, None),
         ("thin2_c40", "thin2", 4.0, None), ("big6_c40", "big6", 4.0, None)]


def check(name, n, indices, dist, cutoff, maxn, full_dist_of):
    assert np.all(np.abs(dist - cutoff) > 1e-3), "%s: a distance within 1e-3 of the cutoff" % name
    for i in range(n):
        d = dist[indices[:, 0] == i]
        assert np.all(np.diff(d) >= 0.0), "%s: receiver %d not ascending" % (name, i)
        gaps = np.diff(d)
        assert np.all((gaps > 1e-5) | (gaps < 1e-9)), "%s: receiver %d has distances closer than 1e-5" % (name, i)
        if maxn is not None:
            full = full_dist_of(i)
            if len(full) > maxn:
                assert full[maxn] - full[maxn - 1] > 1e-5, "%s: receiver %d: the cut falls inside a tie" % (name, i)


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from kgcnn.graph.geom import range_neighbour_lattice
    st = structures()
    out = {"names": np.array([c[0] for c in CASES])}
    for name, key, cutoff, maxn in CASES:
        xyz, lat = st[key]
        idx, img, dist = range_neighbour_lattice(xyz.astype(np.float64), lat.astype(np.float64), max_distance=cutoff,
                                                 max_neighbours=maxn, self_loops=False, exclusive=True)
        idx, img, dist = np.asarray(idx, np.int64).reshape(-1, 2), np.asarray(img, np.int64).reshape(-1, 3), \
            np.asarray(dist, np.float64).reshape(-1)
        full = None
        if maxn is not None:
            fi, _, fd = range_neighbour_lattice(xyz.astype(np.float64), lat.astype(np.float64),
                                                max_distance=cutoff + 1.0, max_neighbours=None, self_loops=False,
                                                exclusive=True)
            fi, fd = np.asarray(fi).reshape(-1, 2), np.asarray(fd).reshape(-1)
            full = lambda i: fd[fi[:, 0] == i]
        check(name, len(xyz), idx, dist, cutoff, maxn, full)
        assert np.all(np.diff(idx[:, 0]) >= 0), "%s: receivers not in node order" % name
        deg = np.bincount(idx[:, 0], minlength=len(xyz))
        print("%-14s N=%d M=%d degrees %d..%d max |image| %d" % (name, len(xyz), len(idx), deg.min(), deg.max(),
                                                                 int(np.abs(img).max()) if len(img) else 0))
        if name == "tri5_c40":
            assert deg.max() < 64
        if name == "tri5_c46":
            assert 64 < deg.min() and deg.max() < 128
        if name == "tri5_c55":
            assert deg.max() > 128 and deg.max() < 1024
        if name == "tri5_c40_n12":
            assert min(full(i)[12] - full(i)[11] for i in range(len(xyz))) >= 2e-3
        if name == "unwrapped_c40":
            assert len(idx) == len(out["indices_tri5_c40"]) and np.abs(img).max() >= 3
        if name == "big6_c40":
            assert deg.min() == 0 and deg.max() > 0
        out["xyz_" + name], out["lattice_" + name] = xyz, lat
        out["cutoff_" + name], out["maxn_" + name] = np.float64(cutoff), np.int64(-1 if maxn is None else maxn)
        out["indices_" + name], out["images_" + name], out["dist_" + name] = idx, img, dist
    path = os.path.join(HERE, "periodic_cases.npz")
    np.savez_compressed(path, **out)
    print("cases:", len(CASES), "arrays:", len(out), "fixture bytes:", os.path.getsize(path))

    from gcnn_keras_amd.synth import periodic_structures
    b = periodic_structures(128)
    ns = b["node_splits"]
    for cutoff in (4.0, 5.0):
        best, edges = None, 0
        for rep in range(3):
            t0 = time.perf_counter()
            edges = 0
            for g in range(len(ns) - 1):
                r = range_neighbour_lattice(b["node_coordinates"][ns[g]:ns[g + 1]].astype(np.float64),
                                            b["graph_lattice"][g].astype(np.float64), max_distance=cutoff,
                                            max_neighbours=None, self_loops=False, exclusive=True)
                edges += len(r[0])
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        print("reference NumPy, 128 structures (N=%d), cutoff %.1f: %.1f ms (best of 3), %d edges"
              % (int(ns[-1]), cutoff, best * 1e3, edges))


if __name__ == "__main__":
    main()
