"""The command line of the analysis tools: key=value arguments, the usage refusal, true|false options, the `[tool] message` report of an
error the tool names, and the files a tool writes.  A tool's `main` is: parse, call its function form, write and print its summary line."""
from __future__ import annotations

import os
import sys

from .. import h5lite


def split(argv, options) -> tuple:
    """(the key=value arguments whose key is one of `options`, every other argument in order); a repeated key keeps its last value."""
    opts = dict(a.split("=", 1) for a in argv if "=" in a and a.split("=", 1)[0] in options)
    return opts, [a for a in argv if not ("=" in a and a.split("=", 1)[0] in opts)]


def parse(argv, options, required, usage, extra_ok=None):
    """-> the options of `argv` (None: sys.argv[1:]) as a dict, or None after printing `usage`: for an argument without `=`, an unknown or a
    repeated key, a missing one of `required`, or where `extra_ok(opts)` is false."""
    argv = list(sys.argv[1:] if argv is None else argv)
    opts, _ = split(argv, options)
    if any(o not in opts for o in required) or len(opts) != len(argv) or (extra_ok is not None and not extra_ok(opts)):
        print(usage, file=sys.stderr)
        return None
    return opts


def flag(opts, name, default="false") -> bool:
    v = opts.get(name, default).lower()
    if v not in ("true", "false"):
        raise ValueError(f"{name} must be true or false (got {opts[name]})")
    return v == "true"


def report(tool, exc) -> int:
    """Print the message of an exception the tool catches as `[tool] message`; -> the exit status 2."""
    print(f"[{tool}] {exc.args[0] if exc.args else exc}", file=sys.stderr)
    return 2


def write(out, tree) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    h5lite.write_tree(out, tree)


def write_clips(directory, trees) -> None:
    """<directory>/clip_<c>.h5 for every {c: tree}: a directory the tools take like a roll-out directory."""
    os.makedirs(directory, exist_ok=True)
    for c, tree in trees.items():
        h5lite.write_tree(os.path.join(directory, f"clip_{c}.h5"), tree)
