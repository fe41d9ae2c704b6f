#!/usr/bin/env python3
"""Writes tests/golden/rodent_xml_actuators.npz: the actuator parameters of the reference's rodent.xml
(track_mjx/environment/walker/assets/rodent/rodent.xml) read straight from the XML with ElementTree, for
tests/test_position_walker_cpu.py::test_pos080_blob_actuators_against_the_xml (the position-actuator walker keeps them as written).

  actuator_name            every <actuator> child's name
  actuator_gainprm         its `gainprm` attribute, first three values (missing values 0), float64
  actuator_biasprm         its `biasprm` attribute, first three values (missing values 0), float64
  actuator_biastype        its `biastype` attribute ("none" where absent)
  actuator_gear            first value of its `gear` attribute (1 where absent), float64
  actuator_target          the joint or tendon it drives;  actuator_is_tendon: 1 for a tendon transmission

The values are the elements' own attributes: every rodent actuator spells out gainprm / biasprm / biastype itself.

Run: python tests/golden/make_rodent_xml_actuators.py <path to rodent.xml>   (deterministic; commit the .npz file)
"""
import sys
import xml.etree.ElementTree as ET
from pathlib import Path

import numpy as np


def _first3(s):
    v = [float(x) for x in (s or "").split()][:3]
    return v + [0.0] * (3 - len(v))


def main(xml: str) -> None:
    root = ET.parse(xml).getroot()
    acts = list(root.find("actuator"))
    for a in acts:
        assert a.get("gainprm") is not None and a.get("biasprm") is not None, a.get("name")
    out = Path(__file__).resolve().parent / "rodent_xml_actuators.npz"
    np.savez(out,
             actuator_name=np.array([a.get("name") for a in acts]),
             actuator_gainprm=np.array([_first3(a.get("gainprm")) for a in acts], dtype=np.float64),
             actuator_biasprm=np.array([_first3(a.get("biasprm")) for a in acts], dtype=np.float64),
             actuator_biastype=np.array([a.get("biastype", "none") for a in acts]),
             actuator_gear=np.array([float(a.get("gear", "1").split()[0]) for a in acts], dtype=np.float64),
             actuator_target=np.array([a.get("joint") or a.get("tendon") for a in acts]),
             actuator_is_tendon=np.array([a.get("tendon") is not None for a in acts], dtype=np.int32))
    print(f"wrote {out}: {len(acts)} actuators")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
