#!/usr/bin/env python3
"""Writes tests/golden/rodent_xml.npz: the numbers tests/test_model_compiler.py::test_rodent_blob_scaling_against_the_xml checks the committed
model blob against, read straight from the reference's rodent.xml (track_mjx/environment/walker/assets/rodent/rodent.xml) with ElementTree.

  body_name / body_pos               every <body>'s name and `pos` attribute (default "0 0 0"), unscaled, float64
  actuator_name / actuator_forcerange every <actuator> child's name and `forcerange` attribute (NaN NaN where the element has none)

Run: python tests/golden/make_rodent_xml_fixture.py <path to rodent.xml>   (deterministic; commit the .npz file)
"""
import sys
import xml.etree.ElementTree as ET
from pathlib import Path

import numpy as np


def main(xml: str) -> None:
    root = ET.parse(xml).getroot()
    bodies = list(root.iter("body"))
    acts = list(root.find("actuator"))
    out = Path(__file__).resolve().parent / "rodent_xml.npz"
    np.savez(out,
             body_name=np.array([b.get("name") for b in bodies]),
             body_pos=np.array([[float(v) for v in b.get("pos", "0 0 0").split()] for b in bodies], dtype=np.float64),
             actuator_name=np.array([a.get("name") for a in acts]),
             actuator_forcerange=np.array([[float(v) for v in a.get("forcerange").split()] if a.get("forcerange") is not None else [np.nan, np.nan]
                                           for a in acts], dtype=np.float64))
    print(f"wrote {out}: {len(bodies)} bodies, {len(acts)} actuators")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
