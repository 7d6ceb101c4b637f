"""The ctypes table of ops/_hip.py against the `extern "C"` declarations of csrc/ (no GPU, no built library).

`_SIGS` and `_RESTYPES` restate every launcher's signature by hand; ctypes converts whatever it is told,
so an `int` that became a `long`, or an argument added on one side only, would pass garbage with no
error.  This parses the declarations (definitions and prototypes alike) and compares.
"""
import ctypes
import glob
import os
import re

from ai_agent_kubectl_amd.build import CSRC
from ai_agent_kubectl_amd.ops import _hip

# exports that only other csrc files (or the bench tools) call: not bound, so not in the table
CXX_ONLY = ("ka_gemm_big_splitk", "ka_gemm_big_argmax_ws", "ka_splitk_reduce_launch")

SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "long": ctypes.c_long, "size_t": ctypes.c_size_t}
DECL = re.compile(r'extern\s+"C"\s+([\w\s\*]+?)\b(ka_\w+)\s*\(([^)]*)\)')


def strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def kind(ctype):
    """ctypes type of a C parameter or return type (its name, if any, already removed); None for void."""
    t = " ".join(ctype.replace("const", " ").replace("__restrict__", " ").split())
    if "*" in t or t == "hipStream_t":
        return ctypes.c_void_p
    if t == "void":
        return None
    if t not in SCALARS:
        raise AssertionError(f"C type {ctype.strip()!r} has no ctypes mapping here: add one consciously")
    return SCALARS[t]


def declarations(text):
    """[(name, return kind, [argument kinds])] of every `extern "C" <ret> ka_*(<args>)` in text."""
    out = []
    for ret, name, args in DECL.findall(strip_comments(text)):
        params = [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []
        # a parameter is `<type> <name>`: the type is everything before the last identifier
        kinds = [kind(re.sub(r"\w+$", "", p)) for p in params]
        assert None not in kinds, f"{name}: a void parameter"
        out.append((name, kind(ret), kinds))
    return out


def mismatches(decls, sigs, restypes):
    """Human-readable differences between parsed declarations and a ctypes table (empty: they agree)."""
    bad = []
    for name, ret, kinds in decls:
        if name not in sigs:
            continue
        if kinds != list(sigs[name]):
            bad.append(f"{name}: csrc arguments {[k.__name__ for k in kinds]} != table {[k.__name__ for k in sigs[name]]}")
        want = restypes.get(name, ctypes.c_int)
        if ret is not want:   # void (None) never equals a table entry: bound names return int or size_t
            bad.append(f"{name}: csrc returns {getattr(ret, '__name__', 'void')}, table says {want.__name__}")
    return bad


def csrc_declarations():
    decls = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            decls += declarations(f.read())
    return decls


def test_ctypes_table_matches_csrc():
    decls = csrc_declarations()
    names = {d[0] for d in decls}
    assert len(names) >= len(_hip._SIGS), f"parsed only {len(names)} exports (parser out of date?)"
    assert not set(_hip._SIGS) - names, f"bound but not declared in csrc: {sorted(set(_hip._SIGS) - names)}"
    assert not set(_hip._RESTYPES) - set(_hip._SIGS), "a return type for a name that is not bound"
    # every occurrence (definition and prototypes) is compared, so they also agree with each other
    assert mismatches(decls, _hip._SIGS, _hip._RESTYPES) == []
    assert names - set(_hip._SIGS) == set(CXX_ONLY), "a ka_* export is neither bound nor listed as C++-only"
    by_name = {}
    for name, ret, kinds in decls:   # the unbound ones have no table to agree with: against each other
        assert by_name.setdefault(name, (ret, kinds)) == (ret, kinds), f"{name}: declarations disagree"


def test_comparator_reports_doctored_declarations():
    with open(os.path.join(CSRC, "gemm_skinny.hip")) as f:
        m = re.search(r'extern\s+"C"\s+int\s+ka_gemm_skinny\s*\([^)]*\)', strip_comments(f.read()))
    real = m.group(0)
    assert "\n" in real   # an argument list that spans lines
    assert mismatches(declarations(real), _hip._SIGS, _hip._RESTYPES) == []
    widened = re.sub(r"\bint M\b", "long M", real)
    shorter = re.sub(r",\s*hipStream_t\s+\w+\s*\)", ")", real)
    returns = real.replace("int ka_gemm_skinny", "size_t ka_gemm_skinny")
    for doctored in (widened, shorter, returns):
        assert doctored != real
        bad = mismatches(declarations(doctored), _hip._SIGS, _hip._RESTYPES)
        assert len(bad) == 1 and bad[0].startswith("ka_gemm_skinny:"), bad
    try:
        declarations(real.replace("int M", "unsigned M"))
    except AssertionError as e:
        assert "no ctypes mapping" in str(e)
    else:
        raise AssertionError("an unmapped parameter type was accepted")
