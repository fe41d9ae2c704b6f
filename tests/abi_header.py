"""The prototypes of include/tmjx.h, parsed: what tests/test_abi.py compares hip.SIGNATURES with, and where tests/hostemu finds the parameter names
of an entry point."""
from __future__ import annotations

import functools
import re
from pathlib import Path

HEADER = Path(__file__).resolve().parents[1] / "include" / "tmjx.h"
# scalar C type -> (class, bytes)
SCALARS = {"int": ("int", 4), "int32_t": ("int", 4), "uint32_t": ("int", 4), "unsigned": ("int", 4), "unsigned int": ("int", 4), "int64_t": ("int", 8),
           "uint64_t": ("int", 8), "long long": ("int", 8), "size_t": ("int", 8), "float": ("float", 4), "double": ("float", 8)}


@functools.lru_cache(None)
def prototypes() -> dict:
    """{function: (return type, [(type, name), ...])} of every tmjx_* function the header declares, comments stripped; a pointer's type ends in '*',
    `const` is dropped, and `(void)` is an empty list."""
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(tmjx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = []
        for p in (q.strip() for q in params.split(",")):
            if p in ("", "void"):
                continue
            m = re.fullmatch(r"(.*?)(\w+)\s*(\[[^\]]*\])?", p, re.S)
            ctype = re.sub(r"\bconst\b", " ", m.group(1)).replace("*", " * ").split()
            args.append((" ".join(t for t in ctype if t != "*") + "*" * (ctype.count("*") + bool(m.group(3))), m.group(2)))
        rtype = re.sub(r"\bconst\b", " ", ret).replace("*", " * ").split()
        out[name] = (" ".join(t for t in rtype if t != "*") + "*" * rtype.count("*"), args)
    return out


def parameter_names(name: str) -> list:
    return [n for _, n in prototypes()[name][1]]
