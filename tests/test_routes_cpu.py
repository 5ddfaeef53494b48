"""Host routing against the record in tests/golden/route_sizes.json (tests/golden/make_route_sizes.py wrote it with the
library of the commit BEFORE the size queries became dry runs of the launch ladders).

A size query builds the launch's problem with null tensors and walks the launch's own ladder, so its answer is what the
launch writes.  Held here, per arithmetic mode (one subprocess each) and once with AGCN_WS_SPLIT=2:
  * every slot / tile count equals the recorded one,
  * every workspace is 0 < new <= recorded,
except for the two kinds of difference below, each of which is checked for what it claims rather than waved through.

Kind "narrow": 9 taps, stride 2, at most 64 output channels, default or bf16 mode.  The record assumed the 512-position
tile; the launch refuses it for a stride-2 window ((tt-1)*2+9 frames exceed its 768-float row or its LDS) and falls
through to the 256-position tile, which writes MORE slots than the record said (the overrun this change removes).  The
new count must be ceil(T_out / min(256 // V, T_out)) and larger than the recorded one.

Kind "refused": the new answer is 0 where the record has a number.  The launch returns AGCN_ERR_UNSUPPORTED for the
shape from a leaf's own window / LDS check or an entry point's shape check, so the recorded number described no launch:
  * agcn_dadj_num_slots, C >= 64 and not a multiple of 64 (entry check of agcn_gcn_dadj);
  * stats tiles of 9 taps, stride 2, V = 32 in f32 mode (launch_cfg: a 736-float window row against 704);
  * weight-gradient workspaces of 9 taps at V = 32 on the exact-f32 kernel (launch_wgrad: row pitch 385 / 481 against
    384 / 448; every mode where the f16x3 tap kernel does not take the shape), and of the 1x1 gradient at 128 -> 256
    channels, V = 32 in bf16 mode (wc_launch_pc: 165,664 bytes of LDS against 163,840).
Checked by calling the entry point itself with placeholder tensors and a ZERO-byte workspace: a refused shape answers
AGCN_ERR_UNSUPPORTED, any shape with a route answers AGCN_ERR_WORKSPACE; neither reaches a HIP call.

What the probe relies on, since its placeholder is a host buffer and the file also runs on GPU machines: every launcher
compares its need with workspace_bytes (here 0) before its first HIP call: every leaf takes the dry run, or makes that
comparison, right after its feasibility checks.  A shape that was wrongly listed would so fail the assertion with -2,
never reach a launch.  The operand maxima are passed so that no entry point starts an absmax pass of its own.
"""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_route_sizes", os.path.join(HERE, "golden", "make_route_sizes.py"))
grid = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(grid)

ERR_UNSUPPORTED = -3
REFUSAL_PROBE = r"""
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
buf = ctypes.create_string_buffer(64)
p = ctypes.cast(buf, ctypes.c_void_p)
P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
out = []
for q, c in json.loads(sys.stdin.read()):
    if q in ("agcn_tconv_stats_tiles", "agcn_conv_stats_tiles"):
        cin, cout, t_out, v, k, s = c[:6]
        pad = c[6] if len(c) > 6 else (k - 1) // 2
        T = (t_out - 1) * s + k - 2 * pad
        f = L.agcn_tconv_fwd
        f.argtypes = [P] * 6 + [Z] + [I] * 8 + [P, P]
        out.append(f(p, p, p, p, p, p, 0, 1, cin, cout, T, v, k, s, pad, p, None))
    elif q == "agcn_dadj_num_slots":
        C, v, T = c
        f = L.agcn_gcn_dadj_ex
        f.argtypes = [P] * 5 + [Z] + [I] * 5 + [P] * 3
        out.append(f(p, p, p, p, p, 0, 1, C, C, T, v, p, p, None))
    elif q in ("agcn_tconv_bwd_weight_workspace", "agcn_conv_bwd_weight_workspace"):
        n, cin, cout, T, v, k, s = c[:7]
        pad = c[7] if len(c) > 7 else (k - 1) // 2
        f = L.agcn_tconv_bwd_weight
        f.argtypes = [P] * 4 + [Z] + [I] * 8 + [P] * 3
        out.append([f(p, p, p, p, 0, n, cin, cout, T, v, k, s, pad, a, a, None) for a in (None, p)])
    else:
        out.append(None)
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def sizes():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    assert os.path.exists(lib.LIB_PATH), "build the library first"
    with open(grid.OUT) as f:
        return json.load(f)["passes"], grid.run_passes(lib.LIB_PATH), lib.LIB_PATH


def _narrow(query, case, mode):
    if query not in ("agcn_conv_stats_tiles", "agcn_tconv_stats_tiles"):
        return None
    cin, cout, t_out, v, taps, stride = case[:6]
    if not (taps == 9 and stride == 2 and cout <= 64 and mode in ("default", "default_ws_split2", "bf16")):
        return None
    tt = min(256 // v, t_out)
    return -(-t_out // tt)


def test_route_sizes_against_record(sizes):
    old, new, lib_path = sizes
    narrow_seen, refused = [], {}
    for mode in grid.PASSES:
        for query, (_, _, kind) in grid.QUERIES.items():
            cs = list(grid.cases(query))
            o, n = old[mode][query], new[mode][query]
            assert len(o) == len(n) == len(cs), (mode, query)
            for case, a, b in zip(cs, o, n):
                where = (mode, query, case, a, b)
                if b == 0 and a > 0:
                    refused.setdefault(mode, []).append((query, list(case)))
                elif kind == "bytes":
                    assert 0 < b <= a, where
                elif a != b:
                    assert b == _narrow(query, case, mode) and b > a, where
                    narrow_seen.append(where)
    # the defect the issue names: 64 -> 64 channels, T_out = 150, V = 25: recorded 8 tiles, the narrow tile writes 15
    assert ("default", "agcn_tconv_stats_tiles", (64, 64, 150, 25, 9, 2, 4), 8, 15) in narrow_seen
    # every zero is a shape the launch itself refuses (both with and without the operand maxima, where it takes them)
    for mode, items in refused.items():
        assert all(q in ("agcn_tconv_stats_tiles", "agcn_conv_stats_tiles", "agcn_dadj_num_slots",
                         "agcn_tconv_bwd_weight_workspace", "agcn_conv_bwd_weight_workspace") for q, _ in items), mode
        env = {k: v for k, v in os.environ.items() if not k.startswith("AGCN_")}
        env.update(grid.PASSES[mode])
        r = subprocess.run([sys.executable, "-c", REFUSAL_PROBE, lib_path], input=json.dumps(items), env=env,
                           capture_output=True, text=True, check=True)
        for (q, c), rc in zip(items, json.loads(r.stdout)):
            codes = rc if isinstance(rc, list) else [rc]
            assert all(code == ERR_UNSUPPORTED for code in codes), (mode, q, c, rc)


def test_queries_answer_zero_outside_their_domain():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    assert L.agcn_tconv_stats_tiles(16, 16, 10, 25, 10, 1, 0) == 0          # 10 taps
    assert L.agcn_conv_stats_tiles(16, 16, 10, 25, 3, 1) == 0               # not a shape agcn_conv_fwd covers
    assert L.agcn_gcn_stats_slots(0, 64, 64, 20, 25) == 0
    assert L.agcn_tconv_bwd_weight_workspace(2, 16, 16, 30, 25, 3, 1, 2) == 0
    assert L.agcn_tconv_workspace(16, 16, 30, 25, 3, 1, 2) == 256           # only the slack


def test_record_is_small():
    assert os.path.getsize(grid.OUT) < 256 * 1024
