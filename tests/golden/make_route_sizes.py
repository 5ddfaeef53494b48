"""Recorded answers of every public size query of the library over a fixed grid: tests/golden/route_sizes.json.

REGENERATE ONLY WHEN ROUTING IS CHANGED ON PURPOSE.  The file is the record of which kernel geometry every shape is
routed to (slot and tile counts) and of how much workspace it is given; tests/test_routes_cpu.py holds the built library
against it.  After a deliberate routing change run

    python tests/golden/make_route_sizes.py

with the library built, and review the diff of the JSON file: that diff IS the routing change.

The arithmetic mode is fixed per process, so every pass runs in a fresh subprocess: AGCN_GEMM unset, f32, bf16x3, bf16,
and one more default pass with AGCN_WS_SPLIT=2.  Values are flat integer arrays in grid order (see `cases`).
"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(ROOT, "2s-agcn_amd", "libagcn_hip.so")
OUT = os.path.join(HERE, "route_sizes.json")

CHANNELS = [(3, 64), (16, 16), (32, 48), (64, 64), (64, 96), (64, 128), (96, 64), (128, 128), (128, 256), (256, 256)]
FRAMES = [8, 40, 300]
JOINTS = [18, 25, 32]
TCONV = [(1, 1, 0), (1, 2, 0), (9, 1, 4), (9, 2, 4), (9, 9, 4), (3, 1, 1), (3, 1, 0), (5, 1, 2), (7, 1, 3), (5, 2, 2),
         (4, 1, 1), (3, 3, 0), (6, 4, 2)]
LEGACY = [(k, s) for k, s, p in TCONV if k in (1, 9) and s in (1, 2) and p == (k - 1) // 2]   # what agcn_conv_* covers
BATCH = [2, 128]
PASSES = {"default": {}, "f32": {"AGCN_GEMM": "f32"}, "bf16x3": {"AGCN_GEMM": "bf16x3"}, "bf16": {"AGCN_GEMM": "bf16"},
          "default_ws_split2": {"AGCN_WS_SPLIT": "2"}}

_I, _Z = ctypes.c_int, ctypes.c_size_t
# query -> (result type, number of int arguments, "slots" or "bytes")
QUERIES = {
    "agcn_conv_stats_tiles": (_I, 6, "slots"),
    "agcn_conv_workspace": (_Z, 6, "bytes"),
    "agcn_conv_bwd_weight_workspace": (_Z, 7, "bytes"),
    "agcn_tconv_stats_tiles": (_I, 7, "slots"),
    "agcn_tconv_workspace": (_Z, 7, "bytes"),
    "agcn_tconv_bwd_weight_workspace": (_Z, 8, "bytes"),
    "agcn_gcn_workspace": (_Z, 4, "bytes"),
    "agcn_gcn_stats_tiles": (_I, 4, "slots"),
    "agcn_gcn_stats_slots": (_I, 5, "slots"),
    "agcn_dadj_num_slots": (_I, 3, "slots"),
    "agcn_gcn_project_bwd_weight_workspace": (_Z, 5, "bytes"),
    "agcn_gcn_unit_infer_workspace": (_Z, 5, "bytes"),
}


def out_frames(T, taps, stride, pad):
    return (T + 2 * pad - taps) // stride + 1


def cases(query):
    """Argument tuples of one query, in the order its array is stored."""
    for cin, cout in CHANNELS:
        for T in FRAMES:
            for V in JOINTS:
                if query == "agcn_conv_stats_tiles":
                    for k, s in LEGACY:
                        yield (cin, cout, out_frames(T, k, s, (k - 1) // 2), V, k, s)
                elif query == "agcn_conv_workspace":
                    for k, s in LEGACY:
                        yield (cin, cout, T, V, k, s)
                elif query == "agcn_conv_bwd_weight_workspace":
                    for k, s in LEGACY:
                        for N in BATCH:
                            yield (N, cin, cout, T, V, k, s)
                elif query == "agcn_tconv_stats_tiles":
                    for k, s, p in TCONV:
                        yield (cin, cout, out_frames(T, k, s, p), V, k, s, p)
                elif query == "agcn_tconv_workspace":
                    for k, s, p in TCONV:
                        yield (cin, cout, T, V, k, s, p)
                elif query == "agcn_tconv_bwd_weight_workspace":
                    for k, s, p in TCONV:
                        for N in BATCH:
                            yield (N, cin, cout, T, V, k, s, p)
                elif query in ("agcn_gcn_workspace", "agcn_gcn_stats_tiles"):
                    yield (cin, cout, T, V)
                elif query in ("agcn_gcn_stats_slots", "agcn_gcn_project_bwd_weight_workspace"):
                    for N in BATCH:
                        yield (N, cin, cout, T, V)
                elif query == "agcn_gcn_unit_infer_workspace":
                    for K2 in (0, 64):              # without / with the folded 1x1 second source
                        yield (cin, cout, K2, T, V)
                elif query == "agcn_dadj_num_slots":
                    yield (cin, V, T)
                else:
                    raise KeyError(query)


def evaluate(lib_path):
    """Every query over its cases, in THIS process (whose environment fixes the mode)."""
    L = ctypes.CDLL(lib_path)
    res = {}
    for name, (rtype, nargs, _) in QUERIES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = rtype, [_I] * nargs
        res[name] = [int(fn(*c)) for c in cases(name)]
    return res


def run_passes(lib_path=LIB):
    """{pass name: {query: [values]}}, one fresh subprocess per pass."""
    out = {}
    for name, extra in PASSES.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("AGCN_")}
        env.update(extra)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--eval", lib_path], env=env, capture_output=True,
                           text=True, check=True)
        out[name] = json.loads(r.stdout)
    return out


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--eval":
        json.dump(evaluate(sys.argv[2]), sys.stdout, separators=(",", ":"))
    else:
        lib_path = sys.argv[1] if len(sys.argv) > 1 else LIB
        with open(OUT, "w") as f:
            json.dump({"passes": run_passes(lib_path)}, f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
