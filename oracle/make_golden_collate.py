"""Mint tests/golden/collate_ref.npz: outputs of the reference's own collate-time C++ (grid subsampling, radius neighbours; SURVEY
row f4) on the scenes tests/test_collate_oracle.py and tests/test_collate_gpu.py use, so that those tests hold the oracle and the
kernels to the reference without the reference tree.  Needs oracle/_ref/libref_collate.so (oracle/Makefile, where the reference
sources exist):    python oracle/make_golden_collate.py

Stored per case (keys from the case's parameters, see `sub_key` / `nb_key`): the subsampled points brought to the oracle's canonical
voxel order (the reference emits them in std::unordered_map order) and the per-cloud lengths -- for the 90 000-point cloud a digest of
those points' bytes instead (the tests hold it bit-exact) -- and per row of every neighbour index matrix (padded with len(supports)) a
digest of the row's SORTED indices (`row_digests`).  The reference's rows are in ascending order of distance (asserted here), so a matrix
is the reference's up to the order inside groups of equal distances (tests/test_collate_oracle.py::rows_equal_up_to_ties) exactly when
its row digests equal these and its own rows are in ascending order of distance (`rows_match_reference`).  Only reference OUTPUTS are
stored; inputs are regenerated from diffreg_hip.synth (integer hash)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "diff-reg_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import collate_oracle as co  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "collate_ref.npz")

# (n_src, n_tgt, seed, dl) of the subsampling and of the neighbour cases
SUBSAMPLE = [(1400, 1200, 0, 0.05), (3000, 2500, 1, 0.05), (3000, 2500, 1, 0.1), (700, 900, 2, 0.2)]
NEIGHBORS = [(1400, 1200, 0, 0.05), (3000, 2500, 1, 0.1)]
# the first `limit` columns tests/test_collate_gpu.py compares (stored as their own digests where a row is wider)
LIMITS = {(1400, 1200, 0, 0.05): 40, (3000, 2500, 1, 0.1): 35}
LARGE_DL = 0.037


def digest(a, size=8):
    """`size`-byte BLAKE2b of an array's little-endian bytes, as an unsigned integer"""
    a = np.ascontiguousarray(a)
    return int.from_bytes(hashlib.blake2b(a.astype(a.dtype.newbyteorder("<")).tobytes(), digest_size=size).digest(), "little")


def row_digests(nb):
    """per row of a neighbour index matrix: the 4-byte digest of its indices in ascending order (int32)"""
    srt = np.sort(np.asarray(nb).astype(np.int32), axis=1)
    return np.array([digest(r, 4) for r in srt], np.uint32)


def row_distances(nb, Q, S):
    """float32 squared distance of every entry (the padding index len(S) -> 1e12 and beyond), summed as (x + y) + z"""
    Sx = np.vstack([S, np.full((1, 3), 1e6, np.float32)])
    d = ((Q[:, None, :] - Sx[np.asarray(nb)]) ** 2).astype(np.float32)
    return (d[..., 0] + d[..., 1]) + d[..., 2]


def rows_match_reference(digests, nb, Q, S):
    """`nb` equals the reference's matrix up to the order inside groups of equal distances: the same multiset of indices per row
    and every row in ascending order of distance (as the reference's own rows are)"""
    mine = row_digests(nb)
    assert len(mine) == len(digests), (len(mine), len(digests))
    bad = np.nonzero(mine != digests)[0]
    assert len(bad) == 0, "rows %s differ from the reference's as sets" % bad[:10].tolist()
    unsorted = np.nonzero((np.diff(row_distances(nb, Q, S), axis=1) < 0).any(1))[0]
    assert len(unsorted) == 0, "rows %s are not in ascending order of distance" % unsorted[:10].tolist()
    return True


def sub_key(n_src, n_tgt, seed, dl):
    return "sub_%d_%d_%d_%g" % (n_src, n_tgt, seed, dl)


def nb_key(n_src, n_tgt, seed, dl, j):
    """j = 0: the cloud against itself (r = 1.25 dl), 1: subsampled against the cloud (1.25 dl), 2: the cloud against the subsampled (2.5 dl)"""
    return "nb_%d_%d_%d_%g_%d" % (n_src, n_tgt, seed, dl, j)


def queries(P, L, dl):
    """the three (queries, q_lengths, supports, s_lengths, radius) of a neighbour case, as the tests build them"""
    sp, sl = co.grid_subsample_batch(P, L, dl)
    return ((P, L, P, L, 1.25 * dl), (sp, sl, P, L, 1.25 * dl), (P, L, sp, sl, 2.5 * dl))


def large_cloud():
    """the 90 000-point cloud of tests/test_collate_gpu.py::test_grid_subsample_large_cloud_and_negative_coordinates"""
    from diffreg_hip import synth
    u = synth.hash_uniform(11, 3, (90000, 3), -1.0, 1.0)
    P = np.stack([3.1 * u[:, 0], 2.3 * u[:, 1], 0.4 * np.sin(2 * u[:, 0]) + 0.05 * u[:, 2]], 1).astype(np.float32)
    return P, np.array([50000, 40000], np.int32)


def main():
    from tests.test_collate_oracle import scene
    assert co.ref_lib() is not None, "oracle/_ref/libref_collate.so is not built (make -C oracle)"
    out = {}
    for case in SUBSAMPLE:
        P, L = scene(*case[:3])
        rp, rl = co.ref_subsample_batch(P, L, case[3])
        out[sub_key(*case) + "_points"] = rp[co.canonical_order(rp, rl, P, L, case[3])]
        out[sub_key(*case) + "_lengths"] = rl
    for case in NEIGHBORS:
        P, L = scene(*case[:3])
        for j, (Q, ql, S, sl_, r) in enumerate(queries(P, L, case[3])):
            rn = co.ref_batch_query(Q, S, ql, sl_, r)
            assert (np.diff(row_distances(rn, Q, S), axis=1) >= 0).all()
            out[nb_key(*case, j)] = row_digests(rn)
            if rn.shape[1] > LIMITS[case]:
                out[nb_key(*case, j) + "_first%d" % LIMITS[case]] = row_digests(rn[:, :LIMITS[case]])
    P, L = large_cloud()
    rp, rl = co.ref_subsample_batch(P, L, LARGE_DL)
    out["sub_large_points_digest"] = np.array([digest(rp[co.canonical_order(rp, rl, P, L, LARGE_DL)])], np.uint64)
    out["sub_large_lengths"] = rl
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %.2f MB uncompressed, %.2f MB on disk" % (OUT, len(out), sum(a.nbytes for a in out.values()) / 1e6,
                                                                      os.path.getsize(OUT) / 1e6))


if __name__ == "__main__":
    main()
