"""CPU checks of the drop-in boundary: the C-ABI library loads without a GPU and exports exactly the symbols that
include/agcn_hip.h declares and 2s-agcn_amd/lib.py binds (no compute calls here); the header is the one declaration:
the sources are compiled against it, the binding table is parsed from it, and lib.call / lib.status convert their
arguments by it."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'agcn_hip.h')


def header_symbols():
    text = open(os.path.join(ROOT, 'include', 'agcn_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(agcn_[a-z0-9_]+)\s*\(', text)))


def test_header_matches_binding_table():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    assert header_symbols() == sorted(lib.SIGNATURES.keys())


def test_library_loads_and_exports_every_symbol():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in header_symbols():
        assert hasattr(handle, name), name
    L = lib.load()
    assert L.agcn_arch() == b'gfx950'
    assert L.agcn_version() >= 100
    # host-only geometry queries
    assert L.agcn_conv_tile_frames(25, 300) == 10 and L.agcn_conv_num_tiles(25, 300) == 30
    assert L.agcn_conv_num_tiles(18, 300) == 22 and L.agcn_scores_num_tiles(25, 75) == 8
    assert L.agcn_dadj_num_slots(3, 25, 300) == 60          # f32 path: 5-frame tiles
    assert L.agcn_dadj_num_slots(64, 25, 300) in (75, 60)   # chained bf16x6 path: 4-frame tiles at 64 channels (AGCN_GEMM default)
    assert L.agcn_conv_bwd_weight_workspace(128, 64, 64, 300, 25, 9, 1) > 0


def test_argument_errors_are_reported_not_thrown():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    L = lib.load()
    # null pointers / bad sizes are rejected on the host before any launch (no GPU needed)
    assert L.agcn_conv_fwd(None, None, None, None, None, None, 0, 1, 1, 1, 1, 25, 9, 1, None) == -1
    assert L.agcn_bn_act_fwd(None, None, None, None, None, None, None, None, 1, 1, 1, 0, 1, None) == -1
    assert L.agcn_adjacency_fwd(None, None, None, None, None, None, None, 1, 1, 1, 25, None) == -1


def test_missing_extension_fails_loudly(tmp_path, monkeypatch):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    monkeypatch.setattr(lib, '_lib', None)
    monkeypatch.setattr(lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        lib.load()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, '2s-agcn_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle|import_module\(.oracle|/oracle', src, flags=re.M), \
                    os.path.join(dirpath, f)


# ---- one declaration: the table is the header's text ------------------------------------------------------------------
_P, _I, _F, _D, _Z, _L = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t,
                          ctypes.c_long)
# written out by hand (they were rows of the literal table this binding used to carry); together they hold every
# return kind, every scalar kind and a pointer of every element kind
PINNED = {
    "agcn_arch": (ctypes.c_char_p, []),
    "agcn_conv_workspace": (_Z, [_I, _I, _I, _I, _I, _I]),
    "agcn_absmax": (_I, [_P, _L, _P, _P]),
    "agcn_bn_stats_finalize": (_I, [_P, _I, _I, _D, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P]),
    "agcn_sgn_collate": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P]),
    "agcn_sgn_stats_finalize": (_I, [_P, _Z, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _Z, _P]),
}


@pytest.mark.parametrize('name', sorted(PINNED))
def test_derived_signature_matches_the_pinned_one(name):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    res, args = lib.SIGNATURES[name]
    assert res is PINNED[name][0]
    assert list(args) == PINNED[name][1]


def test_declared_element_types_and_error_codes():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib, ops
    ret, params = lib.DECLARATIONS["agcn_sgn_collate"]
    assert ret == "int"
    assert params[:7] == [("const float*", "pool"), ("const long long*", "index"), ("const unsigned*", "r"),
                          ("const float*", "angles"), ("float*", "out"), ("float*", "subj"), ("int*", "L")]
    assert params[7] == ("long", "P") and params[-1] == ("void*", "stream")
    assert lib.DECLARATIONS["agcn_sgn_stats_finalize"][1][7:9] == [("const double*", "carry_in"),
                                                                  ("double*", "carry_out")]
    assert lib.DECLARATIONS["agcn_mha_fwd"][1][1] == ("const unsigned char*", "null_tok")
    assert (lib.ERR_ARG, lib.ERR_WORKSPACE, lib.ERR_UNSUPPORTED) == (-1, -2, -3)
    assert ops.ERR_UNSUPPORTED == -3


def test_header_parser_is_strict():
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    with pytest.raises(RuntimeError, match='agcn_f'):
        lib.parse_header("int agcn_f(short n, void* stream);")                # a type outside the closed set
    for unnamed in ("int agcn_f(int, void* stream);", "int agcn_f(const float*, void* stream);",
                    "int agcn_f(const unsigned char* keep, unsigned char);"):
        with pytest.raises(RuntimeError, match='agcn_f'):
            lib.parse_header(unnamed)
    with pytest.raises(RuntimeError, match='agcn_f'):
        lib.parse_header("int agcn_f(int (*callback)(int), void* stream);")   # not a declaration it can read
    with pytest.raises(RuntimeError, match='agcn_f'):
        lib.parse_header("short agcn_f(int n);")                              # return type outside the set
    # comments hold semicolons and parentheses; preprocessor lines and the extern "C" braces are not declarations
    text = '''/* prose; with (parentheses); */
#ifdef __cplusplus
extern "C" {
#endif
#define AGCN_ERR_ARG (-1) /* null pointer; V > 32 (say) */
size_t agcn_q(int W);   // bytes; (a query)
int agcn_f(const float* x /* (N, C); fp32 */, long n,
           void* scratch /* agcn_q(2*C); */, void* stream);   /* enqueues; returns a status */
#ifdef __cplusplus
}
#endif
'''
    decls, codes = lib.parse_header(text)
    assert decls == {"agcn_q": ("size_t", [("int", "W")]),
                     "agcn_f": ("int", [("const float*", "x"), ("long", "n"), ("void*", "scratch"),
                                        ("void*", "stream")])}
    assert codes == {"AGCN_ERR_ARG": -1}


def test_missing_header_fails_loudly(tmp_path, monkeypatch):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    monkeypatch.setattr(lib, 'HEADER_PATH', str(tmp_path / 'nope.h'))
    with pytest.raises(RuntimeError, match='header'):
        lib._read_header()


def test_header_compiles_as_c99():
    cc = next((c for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip('no host C compiler')
    r = subprocess.run([cc, '-std=c99', '-Wall', '-Wstrict-prototypes', '-Werror', '-fsyntax-only', '-x', 'c', HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def _host_syntax_check(tmp_path, name, definition):
    import __graft_entry__ as g
    src = tmp_path / name
    src.write_text('#include "%s"\n%s\n' % (os.path.join(g.CSRC, 'agcn_common.h'), definition))
    return subprocess.run([g.HIPCC, '--offload-arch=gfx950', '-std=c++17', '--cuda-host-only', '-fsyntax-only',
                           str(src)], capture_output=True, text=True)


def test_a_definition_that_drifts_from_the_header_does_not_compile(tmp_path):
    """Every source that defines an entry point includes agcn_common.h, which includes the public header: the compiler
    holds each definition against its declaration."""
    good = _host_syntax_check(tmp_path, 'good.hip', 'extern "C" int agcn_version(void) { return 100; }')
    assert good.returncode == 0, good.stderr[-2000:]
    bad = _host_syntax_check(tmp_path, 'bad.hip', 'extern "C" {\nint agcn_version(int) { return 100; }\n}')
    assert bad.returncode != 0 and 'conflicting types' in bad.stderr, bad.stderr[-2000:]


# ---- lib.call / lib.status: everything that can be refused on the host is, without a GPU ------------------------------
def test_call_refuses_a_cpu_tensor_and_a_wrong_argument_count(monkeypatch):
    import torch
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    reached = []
    monkeypatch.setattr(lib, 'stream', lambda: reached.append(1))    # read only once every argument is converted
    x = torch.zeros(1024)
    for fn in (lib.call, lib.status):
        with pytest.raises(RuntimeError, match=r'agcn_absmax\(x\).*GPU tensor'):
            fn("agcn_absmax", x, 1024, None)
        with pytest.raises(RuntimeError, match=r'agcn_absmax\(out\).*GPU tensor'):
            fn("agcn_absmax", None, 1024, x)
        with pytest.raises(RuntimeError, match='agcn_absmax takes 3 arguments'):
            fn("agcn_absmax", None, 1024)
        with pytest.raises(RuntimeError, match='agcn_absmax takes 3 arguments'):
            fn("agcn_absmax", None, 1024, None, None)                 # the stream is not the caller's to pass
        with pytest.raises(RuntimeError, match='agcn_conv_workspace is not a stream entry point'):
            fn("agcn_conv_workspace", 64, 64, 300, 25, 9, 1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        lib.ptr(x)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        lib.ptr_bits(torch.zeros(4, dtype=torch.int32))
    assert lib.ptr(None) is None and not reached


def test_status_returns_the_code_and_call_raises_with_the_name(monkeypatch):
    import agcn_amd  # noqa: F401
    from agcn_amd import lib
    monkeypatch.setattr(lib, 'stream', lambda: None)     # no GPU here; the null-pointer check comes before any HIP call
    args = (None, None, None, None, 1e-5, 1, None, None, None, None)
    assert lib.status("agcn_bn_eval_coeff_ex", *args) == lib.ERR_ARG
    with pytest.raises(RuntimeError, match=r'agcn_bn_eval_coeff_ex failed with code -1'):
        lib.call("agcn_bn_eval_coeff_ex", *args)
