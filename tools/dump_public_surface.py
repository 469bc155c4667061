#!/usr/bin/env python3
"""The public surface of the Python binding as JSON: what tests, tools and bench.py can reach by name.

    python tools/dump_public_surface.py > tests/public_surface.json

One line per name: its kind, its ``inspect.signature`` and a digest of its docstring (a function, a property, a class), or its
value (a constant).  ``registration`` lists every public name; the package lists its own and describes only those that are not
``registration``'s object of that name.  Every public class lists its public attributes and the non-public ones tests and tools
use (``PRIVATE_USED``), inherited ones included, except what it has unchanged from its nearest public base, which is named.
Where a name is defined is not recorded: moving code between modules leaves the dump unchanged, changing what a caller sees does
not.  Importing the package does not load the library, so this runs without a build and without a GPU.
tests/test_python_binding.py compares the committed dump with the one of the tree it runs in."""
import hashlib
import inspect
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIVATE_USED = ("__init__", "__del__", "_check", "_set", "_occ_info", "_pose_args", "_frame_begin")


def _callable(kind, f):
    try:
        sig = str(inspect.signature(f))
    except (TypeError, ValueError):
        sig = "(?)"
    doc = inspect.getdoc(f)
    return "%s %s doc:%s" % (kind, sig, hashlib.sha256(doc.encode()).hexdigest()[:12] if doc else "none")


def _describe(obj) -> str:
    if isinstance(obj, property):
        return _callable("property", obj.fget)
    if isinstance(obj, (staticmethod, classmethod)):
        return _callable(type(obj).__name__, obj.__func__)
    if inspect.isfunction(obj):
        return _callable("function", obj)
    if inspect.isclass(obj):
        return _callable("class", obj)
    return "value " + repr(obj)


def _attributes(cls) -> dict:
    return {name: _describe(inspect.getattr_static(cls, name)) for name in dir(cls) if not name.startswith("_") or name in PRIVATE_USED}


def _public(module) -> dict:
    return {k: v for k, v in vars(module).items()
            if not k.startswith("_") and not isinstance(v, types.ModuleType) and type(v).__module__ != "__future__"}


def surface() -> dict:
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import pointcloud_slam_amd as pkg
    reg, top = _public(pkg.registration), _public(pkg)
    out = {"registration": {k: _describe(v) for k, v in reg.items()},
           "package": {k: "registration's" if reg.get(k) is v else _describe(v) for k, v in top.items()}}
    classes = {k: v for k, v in {**reg, **top}.items() if inspect.isclass(v) and v.__module__.startswith(pkg.__name__)}
    for name, cls in classes.items():
        base = next((b for b in cls.__mro__[1:] if b in classes.values()), None)
        inherited = _attributes(base) if base else {}
        own = {k: v for k, v in _attributes(cls).items() if inherited.get(k) != v}
        out["class " + name] = dict(own, **({"(base)": base.__name__} if base else {}))
    return out


if __name__ == "__main__":
    json.dump(surface(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
