"""CPU: include/mivp.h is the prototype table of the ctypes binding.

1. the header parser of mivp_amd._lib against an independent reading of the header (names, the size_t queries, three
   prototypes written out by hand);
2. every call site in the tree against the table, statically: declared name, positional count, and no hand-made scalar
   wrapper left in the package;
3. with the library built: argtypes / restype on every function, and _lib.call refusing a wrong count or an undeclared
   name before anything reaches C."""
import ast
import ctypes as C
import glob
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mivp.h")
PKG = os.path.join(ROOT, "medical-image-segmentation-with-visual-prompts_amd")
SCALAR_WRAPPERS = {"c_int", "c_int32", "c_uint32", "c_int64", "c_size_t", "c_float", "c_double"}

# call sites with a starred argument cannot be counted: (file, entry).  Any other one fails the test.
STARRED = {
    ("medical-image-segmentation-with-visual-prompts_amd/inference.py", "mivp_window_blend_any"),
    ("medical-image-segmentation-with-visual-prompts_amd/inference.py", "mivp_window_blend_tta"),
    ("medical-image-segmentation-with-visual-prompts_amd/inference.py", "mivp_window_blend"),
    ("medical-image-segmentation-with-visual-prompts_amd/inference.py", "mivp_window_occupancy"),
    ("tests/test_hip_attn_exact.py", "mivp_win_attn_bwd_dq"),
    ("tests/test_hip_attn_exact.py", "mivp_win_attn_bwd_dkv"),
    ("tests/test_hip_attn_exact.py", "mivp_win_attn_bwd_fused"),
    ("tests/test_hip_attn_exact.py", "mivp_win_attn_bwd_prompt"),
}


def _protos():
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib
    return _lib.parse_header()


# ---------------------------------------------------------------------------------------------- 1. the parser
def test_parser_finds_every_declared_name():
    text = open(HEADER).read()
    names = set(re.findall(r"\b(mivp_[a-z0-9_]+)\s*\(", text))      # test_module_surface's reading of the header
    assert set(_protos()) == names


def test_parser_gives_size_t_to_the_size_t_queries():
    text = open(HEADER).read()
    declared = set(re.findall(r"^size_t\s+(mivp_\w+)\s*\(", text, flags=re.M))
    parsed = {n for n, (ret, _) in _protos().items() if ret is C.c_size_t}
    assert parsed == declared
    assert {"mivp_mv_rec_ws", "mivp_mv_heads_ws"} <= parsed


def test_parser_against_three_handwritten_prototypes():
    from mivp_amd import _lib
    P = _protos()
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    assert P["mivp_bn_finalize"] == (C.c_int, [vp, i32, i32, C.c_double, vp, vp, f32, f32, vp, vp, vp, vp, vp, vp])
    assert P["mivp_gemm_tn"] == (C.c_int, [C.POINTER(_lib.GemmTnDesc), vp, vp, vp, C.c_size_t, vp, vp])
    assert P["mivp_token_scores_fwd_multi"] == (C.c_int, [i32, vp, vp, vp, vp, i32, vp, vp, vp])
    assert P["mivp_last_error"] == (C.c_char_p, [])


def test_parser_refuses_a_type_outside_the_vocabulary(tmp_path):
    from mivp_amd import _lib
    bad = tmp_path / "bad.h"
    bad.write_text("int mivp_ok(const float* x, mivp_stream_t stream);\nint mivp_odd(const long double* x);\n")
    with pytest.raises(RuntimeError, match="mivp_odd"):
        _lib.parse_header(str(bad))
    bad.write_text("short mivp_short(void);\n")
    with pytest.raises(RuntimeError, match="mivp_short"):
        _lib.parse_header(str(bad))


# ---------------------------------------------------------------------------------------------- 2. the call sites
def _entry_names(node):
    """the entry names a `call(...)` site can reach: a literal, or a conditional between literals; else None"""
    if isinstance(node, ast.Constant) and isinstance(node.value, str):
        return [node.value]
    if isinstance(node, ast.IfExp):
        a, b = _entry_names(node.body), _entry_names(node.orelse)
        return a + b if a and b else None
    return None


def _mivp_names(args):
    names = _entry_names(args[0]) if args else None
    return names if names and all(e.startswith("mivp_") for e in names) else None


def _sites(tree):
    """(entry names or None, positional argument nodes, line) of every C-ABI call in a module"""
    for n in ast.walk(tree):
        if not isinstance(n, ast.Call):
            continue
        f = n.func
        if isinstance(f, ast.Attribute) and f.attr.startswith("mivp_"):             # ....lib().mivp_x(...)
            yield [f.attr], n.args, n.lineno
        elif isinstance(f, ast.Attribute) and f.attr == "call" and isinstance(f.value, ast.Name) \
                and f.value.id in ("L", "_lib"):                                     # L.call(<anything>, ...)
            yield (_entry_names(n.args[0]) if n.args else None), n.args[1:], n.lineno
        elif (isinstance(f, ast.Name) or isinstance(f, ast.Attribute)) and _mivp_names(n.args) \
                and (f.id if isinstance(f, ast.Name) else f.attr) == "call":         # call("mivp_x", ...) under any alias
            yield _mivp_names(n.args), n.args[1:], n.lineno


def _is_scalar_wrapper(node):
    """C.c_int32(x), ctypes.c_int32(x) or a bare c_int32(x), at any depth of the argument (arrays are (T * n)(...))"""
    for n in ast.walk(node):
        if isinstance(n, ast.Call) and (n.func.attr if isinstance(n.func, ast.Attribute) else
                                        n.func.id if isinstance(n.func, ast.Name) else None) in SCALAR_WRAPPERS:
            return True
    return False


def test_every_call_site_matches_its_prototype():
    P = _protos()
    files = glob.glob(os.path.join(PKG, "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")) + \
        glob.glob(os.path.join(ROOT, "tests", "*.py")) + [os.path.join(ROOT, "bench.py"),
                                                           os.path.join(ROOT, "__graft_entry__.py")]
    errors, seen, starred = [], 0, set()
    for path in sorted(files):
        rel = os.path.relpath(path, ROOT).replace(os.sep, "/")
        with open(path) as fh:
            tree = ast.parse(fh.read())
        for names, args, line in _sites(tree):
            where = f"{rel}:{line}"
            if names is None:
                errors.append(f"{where}: the entry name is not a literal, the call cannot be checked")
                continue
            seen += 1
            fixed = [a for a in args if not isinstance(a, ast.Starred)]
            for name in names:
                if name not in P:
                    errors.append(f"{where}: {name} is not declared in mivp.h")
                    continue
                want = len(P[name][1])
                if len(fixed) != len(args):
                    starred.add((rel, name))
                    if (rel, name) not in STARRED:
                        errors.append(f"{where}: {name} is called with a starred argument and is not listed in STARRED")
                    if len(fixed) > want:
                        errors.append(f"{where}: {name} takes {want} arguments, {len(fixed)} fixed ones given")
                elif len(args) != want:
                    errors.append(f"{where}: {name} takes {want} arguments, {len(args)} given")
            if path.startswith(PKG + os.sep):
                errors += [f"{where}: scalar wrapper {ast.unparse(a)} (argtypes convert plain numbers)"
                           for a in args if _is_scalar_wrapper(a)]
    assert not errors, "\n".join(errors)
    assert seen > 150                                  # the walk found the call sites at all
    assert starred == STARRED                          # and the list above names nothing that is gone


# ---------------------------------------------------------------------------------------------- 3. the loaded library
def test_loaded_library_carries_the_prototypes():
    from mivp_amd import _lib
    lib = _lib.lib()
    for name, (restype, argtypes) in _protos().items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == argtypes, name


def test_call_refuses_a_wrong_count_and_an_undeclared_name():
    from mivp_amd import _lib
    _lib.lib()
    entry = _lib.call          # (another name: the static walk above must not read these malformed calls as call sites)
    nothing = None             # a NULL pointer: were one of these calls to reach C, it would fail with EINVAL or fault
    good = (nothing, 0, 8, nothing, nothing, 0, nothing, nothing)
    assert len(good) == len(_protos()["mivp_affine_act"][1])
    with pytest.raises(TypeError, match=r"mivp_affine_act takes 8 arguments .* 7 given"):
        entry("mivp_affine_act", *good[:-1])
    with pytest.raises(TypeError, match=r"mivp_affine_act takes 8 arguments .* 9 given"):
        entry("mivp_affine_act", *good, nothing)
    with pytest.raises(RuntimeError, match="mivp_no_such_entry is not declared"):
        entry("mivp_no_such_entry", nothing)
    with pytest.raises(C.ArgumentError):               # a descriptor of the wrong kind is refused by its argtype
        entry("mivp_gemm_tn", C.byref(_lib.ConvDesc()), nothing, nothing, nothing, 0, nothing, nothing)
