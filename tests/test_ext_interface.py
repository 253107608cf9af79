"""The python wrapper and the built extension agree on the interface.

CPU-only: the built _flreid_hip imports without a GPU, and nothing here
launches.  Call-arity drift between ops/__init__.py and a binding otherwise
shows only when the call runs on a GPU."""

import ast
import os
import re

import pytest

from flreid_amd import ops

pytestmark = pytest.mark.skipif(not ops.extension_available(),
                                reason="HIP extension not built")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAPPER = os.path.join(REPO, "flreid_amd", "ops", "__init__.py")


def _ext_calls():
    """(name, n_positional, lineno, plain) of every ext.<name>(...) and
    ctx.ext.<name>(...) call in the wrapper; plain = no *args / keywords."""
    with open(WRAPPER) as f:
        tree = ast.parse(f.read())
    calls = []
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call)
                and isinstance(node.func, ast.Attribute)):
            continue
        recv = node.func.value
        if not ((isinstance(recv, ast.Name) and recv.id == "ext")
                or (isinstance(recv, ast.Attribute) and recv.attr == "ext"
                    and isinstance(recv.value, ast.Name)
                    and recv.value.id == "ctx")):
            continue
        plain = not node.keywords and not any(
            isinstance(a, ast.Starred) for a in node.args)
        calls.append((node.func.attr, len(node.args), node.lineno, plain))
    return calls


def _binding_arity(fn) -> int:
    """Parameters in the pybind-generated signature, the docstring's first
    line: `name(arg0: int, arg1: float, ...) -> None`."""
    sig = fn.__doc__.splitlines()[0]
    assert re.match(r"^\w+\(.*\) -> ", sig), sig
    return len(re.findall(r"\barg\d+: ", sig))


def _public_callables(ext):
    return sorted(n for n in dir(ext)
                  if not n.startswith("_") and callable(getattr(ext, n)))


def test_wrapper_calls_match_the_bindings():
    ext = ops._load_extension()
    calls = _ext_calls()
    assert len(calls) >= 30, "the wrapper's ext calls were not found"
    problems = []
    for name, n_args, lineno, plain in calls:
        where = f"ops/__init__.py:{lineno} ext.{name}"
        if not hasattr(ext, name):
            problems.append(f"{where}: no such binding")
        elif not plain:
            problems.append(f"{where}: *args / keyword call, arity unknown")
        elif n_args != _binding_arity(getattr(ext, name)):
            problems.append(f"{where}: {n_args} arguments, the binding "
                            f"takes {_binding_arity(getattr(ext, name))}")
    assert not problems, "\n".join(problems)


def test_every_binding_is_referenced():
    """A binding that neither the wrapper nor benchmarks/ nor tests/ names is
    dead: report it."""
    ext = ops._load_extension()
    text = [open(WRAPPER).read()]
    for sub in ("benchmarks", "tests"):
        for root, _dirs, files in os.walk(os.path.join(REPO, sub)):
            for fn in files:
                path = os.path.join(root, fn)
                if fn.endswith(".py") and path != os.path.abspath(__file__):
                    with open(path) as f:
                        text.append(f.read())
    text = "\n".join(text)
    dead = [n for n in _public_callables(ext)
            if not re.search(rf"\bext\.{n}\b", text)]
    assert not dead, f"bindings nothing references: {dead}"
