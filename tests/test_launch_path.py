"""Every call that puts work on a stream goes through `_native._launch` (no GPU needed): the names it is given are
entry points a plan can hold (`PLAN_FNS` of csrc/plan.hip) with a ctypes signature, no such entry point is called any
other way, and nothing but `load()` sets the module's library handle - the single place where timing and plan
recording see every launch."""

import ast
import os
import re

from conftest import PKG_ROOT


def plan_fns():
    text = open(os.path.join(PKG_ROOT, "csrc", "plan.hip")).read()
    body = text[text.index("PLAN_FNS[] = {"):]
    body = body[: body.index("};")]
    names = set(re.findall(r"BESS_PLAN_FN\((bess_\w+)\)", body))
    assert len(names) >= 40
    return names


def native_tree():
    return ast.parse(open(os.path.join(PKG_ROOT, "besskge", "_native.py")).read())


def launched_names(tree):
    out = []
    callers = [n for n in tree.body if not (isinstance(n, ast.FunctionDef) and n.name == "_launch")]
    for node in (n for top in callers for n in ast.walk(top)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "_launch":
            assert isinstance(node.args[0], ast.Constant), f"line {node.lineno}: _launch needs a literal entry point"
            out.append(node.args[0].value)
    return out


def test_every_launch_names_a_plan_entry_point():
    from besskge import _native

    fns = plan_fns()
    names = launched_names(native_tree())
    assert len(names) >= 50
    for name in names:
        assert name in fns, f"{name} is launched but is not in PLAN_FNS"
        assert name in _native.SIGNATURES, f"{name} is launched but has no ctypes signature"


def test_plan_entry_points_are_called_only_through_launch():
    fns = plan_fns()
    bad = []
    for node in ast.walk(native_tree()):
        # load().bess_x(...), lib.bess_x(...): an attribute named after one
        if isinstance(node, ast.Attribute) and node.attr in fns:
            bad.append(f"line {node.lineno}: .{node.attr}")
        # getattr(lib, "bess_x")
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "getattr" \
                and len(node.args) > 1 and isinstance(node.args[1], ast.Constant) and node.args[1].value in fns:
            bad.append(f"line {node.lineno}: getattr(..., {node.args[1].value!r})")
    assert not bad, bad


def test_only_load_assigns_the_library_handle():
    tree = native_tree()
    offenders = []
    for fn in ast.walk(tree):
        if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            continue
        for node in ast.walk(fn):
            if isinstance(node, ast.Global) and "_lib" in node.names and getattr(fn, "name", "") != "load":
                offenders.append(f"{fn.name} declares `global _lib`")
            if isinstance(node, ast.Attribute) and node.attr == "_lib" and isinstance(node.ctx, ast.Store):
                offenders.append(f"{getattr(fn, 'name', '?')} line {node.lineno} stores an attribute _lib")
    module_level = [n for n in tree.body if isinstance(n, (ast.Assign, ast.AnnAssign))
                    for t in (n.targets if isinstance(n, ast.Assign) else [n.target])
                    if isinstance(t, ast.Name) and t.id == "_lib"]
    assert len(module_level) == 1  # the `_lib = None` declaration
    assert not offenders, offenders


def test_timing_labels_name_entry_points():
    from besskge import _native

    for variant, label in _native.TIMING_LABELS.items():
        assert variant in _native.SIGNATURES, variant
        assert label in _native.SIGNATURES, label
        assert variant in plan_fns(), variant
