#!/usr/bin/env python3
"""Writes tests/golden/rodent_xml_render.npz: what tests/test_render_cpu.py::test_render_side_file_against_the_xml checks the committed render
side files (<stem>.render.tmjx.txt) against, read straight from the reference's rodent.xml with ElementTree (defaults classes resolved here,
independently of tools/compile_model.py).

  geom_name / geom_body / geom_type       every <geom> in document order: its name, its body's name ("world" for worldbody), resolved type
  geom_size [n, 3] / geom_pos [n, 3]      `size` zero padded and `pos` (default "0 0 0"), unscaled, float64
  geom_orient_kind / geom_orient [n, 6]   which orientation attribute the geom resolves to (none | quat | euler) and its values, zero padded
  geom_rgba [n, 4] / geom_group           resolved rgba (MuJoCo's default 0.5 0.5 0.5 1) and group (default 0)
  geom_below_walker                       1 where the geom hangs below the body "walker" (what dm_scale_spec rescales)
  camera_name / camera_body / camera_mode / camera_pos [c, 3] / camera_fovy (default 45)
  camera_orient_kind / camera_orient [c, 6]   xyaxes | zaxis | euler | quat | none and the attribute's values, zero padded

Run: python tests/golden/make_rodent_render_fixture.py <path to rodent.xml>   (deterministic; commit the .npz file)
"""
import sys
import xml.etree.ElementTree as ET
from pathlib import Path

import numpy as np


def defaults(root):
    """class -> tag -> attributes, a nested <default> inheriting from the one around it."""
    out = {}

    def rec(node, inherited, name):
        own = {k: dict(v) for k, v in inherited.items()}
        for ch in node:
            if ch.tag != "default":
                own.setdefault(ch.tag, {}).update(ch.attrib)
        out[name] = own
        for ch in node:
            if ch.tag == "default":
                rec(ch, own, ch.get("class"))

    for d in root.findall("default"):
        rec(d, out.get("main", {}), d.get("class", "main"))
    return out


def main(xml: str) -> None:
    root = ET.parse(xml).getroot()
    dflt = defaults(root)
    geoms, cams = [], []

    def resolved(el, childclass):
        a = dict(dflt.get(el.get("class", childclass or "main"), {}).get(el.tag, {}))
        a.update({k: v for k, v in el.attrib.items() if k != "class"})
        return a

    def walk(body, name, childclass, below):
        for ch in body:
            if ch.tag == "geom":
                geoms.append((resolved(ch, childclass), name, below))
            elif ch.tag == "camera":
                cams.append((resolved(ch, childclass), name))
        for ch in body:
            if ch.tag == "body":
                walk(ch, ch.get("name"), ch.get("childclass", childclass), below or body.get("name") == "walker")

    wb = root.find("worldbody")
    walk(wb, "world", None, False)

    def vec(s, n):
        v = [float(x) for x in s.split()] if s else []
        return (v + [0.0] * n)[:n]

    def orient(a, kinds):
        for k in kinds:
            if k in a:
                return k, vec(a[k], 6)
        return "none", [0.0] * 6

    go = [orient(a, ("quat", "euler")) for a, _, _ in geoms]
    co = [orient(a, ("quat", "xyaxes", "zaxis", "euler")) for a, _ in cams]
    out = Path(__file__).resolve().parent / "rodent_xml_render.npz"
    np.savez(out,
             geom_name=np.array([a.get("name", "") for a, _, _ in geoms]), geom_body=np.array([b for _, b, _ in geoms]),
             geom_type=np.array([a.get("type", "sphere") for a, _, _ in geoms]),
             geom_size=np.array([vec(a.get("size"), 3) for a, _, _ in geoms], dtype=np.float64),
             geom_pos=np.array([vec(a.get("pos"), 3) for a, _, _ in geoms], dtype=np.float64),
             geom_orient_kind=np.array([k for k, _ in go]), geom_orient=np.array([v for _, v in go], dtype=np.float64),
             geom_rgba=np.array([vec(a.get("rgba", "0.5 0.5 0.5 1"), 4) for a, _, _ in geoms], dtype=np.float64),
             geom_group=np.array([int(a.get("group", 0)) for a, _, _ in geoms], dtype=np.int32),
             geom_below_walker=np.array([int(b) for _, _, b in geoms], dtype=np.int32),
             camera_name=np.array([a.get("name", "") for a, _ in cams]), camera_body=np.array([b for _, b in cams]),
             camera_mode=np.array([a.get("mode", "fixed") for a, _ in cams]),
             camera_pos=np.array([vec(a.get("pos"), 3) for a, _ in cams], dtype=np.float64),
             camera_fovy=np.array([float(a.get("fovy", 45.0)) for a, _ in cams], dtype=np.float64),
             camera_orient_kind=np.array([k for k, _ in co]), camera_orient=np.array([v for _, v in co], dtype=np.float64))
    print(f"wrote {out}: {len(geoms)} geoms, {len(cams)} cameras")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
