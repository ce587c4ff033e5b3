#!/usr/bin/env python3
"""Record what the convolution dispatch (csrc/igemm.hip) decides, through its query entry points only: no GPU is needed.

For every geometry of the committed tile table plus the shapes of the GPU kernel tests, under each GEMM arithmetic
(cstp_gemm_set_split_terms 2, 3, 1):
  "tuned": with the table's tiles set -- cstp_conv3d_query_tile for modes 0..3, cstp_conv3d_in_affine_fused for 1, 2, 3 groups,
           cstp_conv3d_bnstats_nsplit and ..._aff for 1 and 2 groups, cstp_conv3d_workspace_bytes;
  "sweep": the same snapshot after pinning each candidate tile of CANDIDATES in turn (with cstp_conv3d_set_tile's return code),
           kept as one SHA-256 per (arithmetic, geometry).

usage: python tools/record_conv_routes.py [--lib libcstp_hip.so] [--rows] [--write]
  prints the record as JSON; --rows keeps the sweep rows next to their digests; --write replaces tests/golden/conv_routes.json.
Run it in a fresh process without CSTP_* variables: dispatch reads several once per process and keeps tiles process-wide."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_routes.json")
TABLE = os.path.join(ROOT, "cstp_amd", "tuned", "gfx950_abi18.json")

# the shapes of tests/test_split_gpu.py (GEOMS, PATCH_GEOMS, STEMS) and tests/test_pack_replay_gpu.py (TPATCH):
# (x shape, k, kernel, stride, padding)
SPATIAL = ((1, 3, 3), (1, 1, 1), (0, 1, 1))
TEST_SHAPES = [
    ((2, 64, 4, 14, 14), 144) + SPATIAL,                                     # GEOMS
    ((2, 144, 4, 14, 14), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
    ((2, 64, 4, 14, 14), 230, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    ((2, 230, 8, 7, 7), 128, (3, 1, 1), (2, 1, 1), (1, 0, 0)),
    ((1, 512, 2, 7, 7), 1152) + SPATIAL,
    ((3, 40, 3, 9, 11), 136, (3, 3, 3), (1, 2, 1), (1, 1, 1)),
    ((6, 96, 1, 1, 1), 40, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ((2, 64, 4, 14, 14), 42, (1, 1, 1), (1, 2, 2), (0, 0, 0)),
    ((6, 192, 1, 1, 1), 128, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
    ((1, 64, 2, 56, 56), 144) + SPATIAL,                                     # PATCH_GEOMS (S1 and S7 are above)
    ((2, 128, 2, 28, 28), 288) + SPATIAL,
    ((3, 40, 3, 9, 11), 136) + SPATIAL,
    ((2, 16, 1, 5, 6), 24) + SPATIAL,
    ((2, 3, 4, 28, 28), 83, (1, 7, 7), (1, 2, 2), (0, 3, 3)),                # STEMS
    ((3, 3, 3, 23, 19), 83, (1, 7, 7), (1, 2, 2), (0, 3, 3)),
    ((1, 3, 6, 20, 20), 64, (7, 7, 7), (1, 2, 2), (3, 3, 3)),
    ((2, 48, 8, 14, 14), 64, (3, 1, 1), (1, 1, 1), (1, 0, 0)),               # TPATCH
]
ARITHMETICS = (2, 3, 1)
NATIVE = [(0, 2, 1, 1), (0, 9, 1, 1)]
GATHER = [(1, 4, 1, 1), (1, 5, 1, 1), (1, 9, 2, 1)]
PATCH = [(2, 4, 1, 1), (2, 4, 2, 1), (2, 8, 1, 1), (2, 9, 1, 1)]
CANDIDATES = {0: NATIVE + GATHER + PATCH, 1: NATIVE + GATHER + PATCH,
              2: [(0, 3, 8, 0), (0, 9, 8, 0), (1, 4, 4, 0), (1, 9, 16, 0), (2, 9, 1, 0)]}


def geometries():
    with open(TABLE) as f:
        tiles = json.load(f)["tiles"]
    table = {}
    for key, tile in tiles.items():
        arith, mode, desc = key.split("|")
        table.setdefault(tuple(int(v) for v in desc.split(",")), {})[(int(arith), int(mode))] = tile
    descs = set(table)
    for xs, k, ks, st, pd in TEST_SHAPES:
        descs.add(tuple(xs) + (k,) + tuple(ks) + tuple(st) + tuple(pd))
    return sorted(descs), table


def snapshot(lib, D):
    row = []
    for mode in range(4):
        t = (ctypes.c_int32 * 4)()
        row.append([lib.cstp_conv3d_query_tile(ctypes.byref(D), mode, t)] + list(t))
    row.append([lib.cstp_conv3d_in_affine_fused(ctypes.byref(D), g) for g in (1, 2, 3)])
    row.append([lib.cstp_conv3d_bnstats_nsplit(ctypes.byref(D), g) for g in (1, 2)] +
               [lib.cstp_conv3d_bnstats_nsplit_aff(ctypes.byref(D), g) for g in (1, 2)])
    row.append(lib.cstp_conv3d_workspace_bytes(ctypes.byref(D)))
    return row


def digest(rows):
    return hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()


def record(lib_path=None, keep_rows=False):
    from cstp_amd import _lib
    if lib_path:
        _lib.LIB_PATH = lib_path
    lib = _lib.load()
    descs, table = geometries()
    out = {"tuned": {}, "sweep": {}}
    if keep_rows:
        out["sweep_rows"] = {}
    for arith in ARITHMETICS:
        lib.cstp_gemm_set_split_terms(arith)
        for desc in descs:
            D = _lib.ConvDesc(*desc)
            name = "%d|%s" % (arith, ",".join(str(v) for v in desc))
            for mode in range(3):
                tile = table.get(desc, {}).get((arith, mode))
                if tile is not None:
                    lib.cstp_conv3d_set_tile(ctypes.byref(D), mode, (ctypes.c_int32 * 4)(*tile))
            out["tuned"][name] = snapshot(lib, D)
            rows = []
            for mode in range(3):
                for cand in CANDIDATES[mode]:
                    rc = lib.cstp_conv3d_set_tile(ctypes.byref(D), mode, (ctypes.c_int32 * 4)(*cand))
                    rows.append([mode, list(cand), rc] + snapshot(lib, D))
            out["sweep"][name] = digest(rows)
            if keep_rows:
                out["sweep_rows"][name] = rows
    lib.cstp_gemm_set_split_terms(0)
    return out


def dumps(rec):
    """One line per geometry (rows stay greppable, the file small)."""
    parts = []
    for sec in sorted(rec):
        body = ",\n".join("%s: %s" % (json.dumps(k), json.dumps(rec[sec][k], separators=(",", ":"))) for k in sorted(rec[sec]))
        parts.append("%s: {\n%s\n}" % (json.dumps(sec), body))
    return "{\n" + ",\n".join(parts) + "\n}\n"


if __name__ == "__main__":
    args = sys.argv[1:]
    lib_path = args[args.index("--lib") + 1] if "--lib" in args else None
    text = dumps(record(lib_path, "--rows" in args))
    if "--write" in args:
        with open(FIXTURE, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
