"""Regenerates tests/golden/angle_cases.npz.  Run ONLY in the build container:

    python -B tests/golden/make_angle_fixtures.py

Source (data only; no reference source text is stored): the node triples and edge pairs that the reference's NumPy-only
``kgcnn.graph.adj.get_angle_indices`` (imported from the reference tree with ``python -B``) returns for five hand-made
edge lists, each for the four edge pairings x ``allow_multi_edges`` x ``allow_reverse_edges`` (``allow_self_edges``
False, ``check_sorted`` True):

0. 14 random edges on 5 nodes with duplicates and self loops, unsorted;
1. the complete directed graph on 4 nodes;
2. the path 0-1-2 in sender order;
3. a single edge;
4. one edge and its reverse.

Keys: ``edges_<c>`` (M, 2) and ``nodes_<c>`` (node count) per case, ``triples_<c>_<pairing>_<multi>_<reverse>`` (A, 3)
and ``pairs_<c>_<pairing>_<multi>_<reverse>`` (A, 2), all int64.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
PAIRINGS = ("jk", "ik", "kj", "ki")


def cases():
    rng = np.random.default_rng(20)
    random14 = rng.integers(0, 5, size=(14, 2)).astype(np.int64)
    random14[5] = random14[2]                 # a duplicate edge
    random14[9] = random14[2][::-1]           # a reverse of it
    random14[11] = (3, 3)                     # a self loop
    random14[12] = (3, 3)                     # ... twice
    complete4 = np.array([(i, j) for i in range(4) for j in range(4) if i != j], dtype=np.int64)
    path = np.array([(1, 0), (0, 1), (2, 1), (1, 2)], dtype=np.int64)
    return [(random14, 5), (complete4, 4), (path, 3), (np.array([(0, 1)], dtype=np.int64), 2),
            (np.array([(0, 1), (1, 0)], dtype=np.int64), 2)]


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    from kgcnn.graph.adj import get_angle_indices
    out = {}
    for c, (edges, nodes) in enumerate(cases()):
        out["edges_%d" % c], out["nodes_%d" % c] = edges, np.int64(nodes)
        for pairing in PAIRINGS:
            for multi in (0, 1):
                for reverse in (0, 1):
                    _, triples, pairs = get_angle_indices(edges, check_sorted=True, allow_multi_edges=bool(multi),
                                                          allow_self_edges=False, allow_reverse_edges=bool(reverse),
                                                          edge_pairing=pairing)
                    key = "%d_%s_%d_%d" % (c, pairing, multi, reverse)
                    out["triples_" + key] = np.asarray(triples, np.int64).reshape(-1, 3)
                    out["pairs_" + key] = np.asarray(pairs, np.int64).reshape(-1, 2)
    path = os.path.join(HERE, "angle_cases.npz")
    np.savez_compressed(path, **out)
    print("cases:", len(cases()), "arrays:", len(out), "fixture bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main()
