"""Records what the size queries of the list, selection and metric entries answer over a fixed argument table ->
tests/golden/workspace_sizes.json.  Pure host calls, no GPU.  The committed file was recorded from a build of the commit BEFORE these entries
moved to one carve per workspace (csrc/carve.h); tests/test_workspace_sizes_cpu.py holds every later build to it.

    python tools/golden/make_golden_workspace_sizes.py [path/to/libdiffreg_hip.so]

TABLE is imported by the test: the table and the recorded file cannot drift apart."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
DEFAULT_LIB = os.path.join(ROOT, "diff-reg_amd", "diffreg_hip", "libdiffreg_hip.so")

I, LL = ctypes.c_int, ctypes.c_longlong
BIG = 1 << 20

# 4-byte arrays cross a 256-byte boundary at 63 / 64 / 65 elements, 8-byte ones at 31 / 32 / 33, 12-byte rows at 21 / 22, 16-byte ones at
# 15 / 16 / 17, CloudInfo rows (36 bytes) at 7 / 8 and 14 / 15, PnpBest rows (104 bytes) at 2 / 3 workgroups = 512 / 513 iterations;
# the sorts pad to a power of two: 64 / 65, 1024 / 1025.
N4 = [1, 31, 32, 33, 63, 64, 65, 1024, 1025]
TABLE = {
    "dr_point_to_node_partition_workspace_bytes": ([I], [(v,) for v in [0, -1] + N4 + [20000]]),
    "dr_unique_pairs_workspace_bytes": ([I], [(v,) for v in [0, -1] + N4 + [60000]]),
    "dr_node_correspondences_2d3d_workspace_bytes": ([I, I, I, LL],
        [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, 5, 4, 15), (3, 5, 4, -2)] +
        [(m, n, kc, cap) for m in (63, 64, 65) for n in (21, 22, 64, 65) for kc in (1, 4) for cap in (15, 63, 64, 65)] +
        [(3, 5, 4, 15), (1, 1, 1, 1), (240, 300, 64, BIG)]),
    "dr_mutual_nn_radius_workspace_bytes": ([I, I],
        [(0, 0), (0, 5), (5, 0), (-1, 5), (5, -1)] + [(a, b) for a in (1, 63, 64, 65, 1025) for b in (1, 3, 63, 64, 65)] + [(5000, 4800)]),
    "dr_radius_pairs_workspace_bytes": ([I, I],
        [(0, 0), (0, 5), (-1, 5), (5, 0), (5, -1)] + [(a, 3) for a in (1, 21, 22, 42, 43, 63, 64, 65, 1024, 1025)] + [(20000, 18000)]),
    "dr_grid_subsample_workspace_bytes": ([I, I],
        [(0, 0), (0, 2), (5, 0), (-1, 2), (5, -1)] +
        [(n, nb) for n in (1, 31, 32, 33, 63, 64, 65, 1024, 1025, 4096, 4097, 262144, 262145) for nb in (1, 2, 7, 8, 14, 15)] + [(60000, 4)]),
    "dr_radius_neighbors_workspace_bytes": ([I, I, I],
        [(0, 0, 0), (7, 0, 2), (7, 65, 0), (7, -1, 2), (7, 65, -1), (0, 65, 2), (-1, 65, 2)] +
        [(7, ns, nb) for ns in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1024, 1025) for nb in (1, 2, 7, 8, 14, 15)] + [(60000, 60000, 4)]),
    "dr_ransac_workspace_bytes": ([I, I, I],
        [(0, 5, 10), (2, 0, 10), (2, 5, 0), (-1, 5, 10), (2, -1, 10), (2, 5, -1)] +
        [(p, cap, it) for p in (1, 2, 3, 15, 16, 17) for cap in (1, 5, 16) for it in (1, 256, 257, 3840, 3841, 4096, 4097)] + [(8, 4096, 50000)]),
    "dr_pnp_ransac_workspace_bytes": ([I, I],
        [(0, 0), (-1, 10), (5, 0), (5, -1), (0, 10)] +
        [(n, it) for n in (4, 5, 255, 256, 257) for it in (1, 256, 257, 512, 513, 1024, 1025)] + [(5000, 5000)]),
    "dr_mutual_topk_workspace_bytes": ([I, I, I],
        [(0, 9, 9), (3, 0, 9), (3, 9, 0), (-1, 9, 9), (3, -1, 9), (3, 9, -1)] +
        [(b, n, m) for b in (1, 3, 63, 64, 65) for (n, m) in ((1, 1), (9, 9), (32, 63), (32, 64), (32, 65), (45, 45), (46, 45), (128, 128))] +
        [(4, 512, 500), (2, 1 << 20, 1 << 20)]),      # (the last: more than 2^31 words per element)
    "dr_procrustes_workspace_bytes": ([I, I, I],
        [(0, 300, 300), (1, 0, 300), (1, 300, 0), (-1, 300, 300), (1, -1, 300), (1, 256, 256)] +
        [(p, n, m) for p in (1, 3, 65) for (n, m) in ((65536, 1), (65537, 1), (257, 256), (1024, 1025), (2048, 2048))] + [(8, 1000, 1200)]),
    "dr_train_workspace_bytes": ([I, I, I],
        [(0, 0, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (0, 5, 5), (1, 0, 5)] +
        [(1, 1, v) for v in (1, 255, 256, 257)] + [(1, 5, 5), (3, 17, 5), (8, 512, 500)]),
}
# (P, N, M, element bytes): one row block (N < 32) answers 0; P * N * 4 straddles a 16-byte boundary at N = 33 .. 36
TABLE["dr_top1_union_workspace_bytes"] = ([I, I, I, I],
    [(0, 4096, 4, 4), (1, 0, 4, 4), (1, 4096, 0, 4), (1, 4096, 4, 2), (-1, 4096, 4, 8), (1, 31, 5, 4)] +
    [(p, n, m, e) for p in (1, 3) for n in (32, 33, 34, 35, 36, 4097) for m in (1, 5, 64) for e in (4, 8)] + [(8, 4096, 4000, 8)])
TABLE["dr_radius_count_hist_workspace_bytes"] = TABLE["dr_radius_neighbors_workspace_bytes"]


def query_all(lib_path):
    lib = ctypes.CDLL(lib_path)
    out = {}
    for name, (argtypes, rows) in sorted(TABLE.items()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_size_t, argtypes
        out[name] = [[list(r), int(fn(*r))] for r in rows]
    return out


if __name__ == "__main__":
    sizes = query_all(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_LIB)
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join('  "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in sizes.items()) + "\n}\n")
    print("wrote %s: %d queries" % (OUT, sum(len(v) for v in sizes.values())))
