#!/usr/bin/env python3
"""Extracts the ORB / camera settings of the reference's example configurations (data, from the text of
Examples/*/*.yaml) into tests/golden/reference_settings.json: the numbers bench.py, the tests and the C examples use for
BASELINE configs 1-5 (nFeatures, scaleFactor, nLevels, iniThFAST, minThFAST, image size, fx, bf).  Build container only."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/Examples"
FILES = {"KITTI00-02 stereo": "Stereo/KITTI00-02.yaml", "TUM1 mono": "Monocular/TUM1.yaml", "EuRoC mono": "Monocular/EuRoC.yaml",
         "EuRoC stereo": "Stereo/EuRoC.yaml"}
KEYS = ("Camera.fx", "Camera.bf", "Camera.width", "Camera.height", "Camera.fps", "ThDepth", "ORBextractor.nFeatures", "ORBextractor.scaleFactor",
        "ORBextractor.nLevels", "ORBextractor.iniThFAST", "ORBextractor.minThFAST")


# the RGB-D sensor (Examples/RGB-D/TUM1-3.yaml) -> tests/golden/reference_settings_rgbd.json: camera, distortion, bf, ThDepth,
# DepthMapFactor and Camera.RGB of Tracking::Tracking (src/Tracking.cc:60-151) -- the constants of tests/test_rgbd.py
RGBD_FILES = {"TUM1 rgbd": "RGB-D/TUM1.yaml", "TUM2 rgbd": "RGB-D/TUM2.yaml", "TUM3 rgbd": "RGB-D/TUM3.yaml"}
RGBD_KEYS = ("Camera.fx", "Camera.fy", "Camera.cx", "Camera.cy", "Camera.k1", "Camera.k2", "Camera.p1", "Camera.p2", "Camera.k3",
             "Camera.width", "Camera.height", "Camera.bf", "Camera.RGB", "ThDepth", "DepthMapFactor", "ORBextractor.nFeatures")
RGBD_JSON = os.path.join(ROOT, "tests", "golden", "reference_settings_rgbd.json")


def parse(path, keys=KEYS):
    return parse_text(open(path, encoding="utf-8", errors="replace").read(), keys)


def parse_text(txt, keys=KEYS):
    out = {}
    for k in keys:
        m = re.search(r"^%s\s*:\s*([-+0-9.eE]+)" % re.escape(k), txt, re.M)
        if m:
            out[k] = float(m.group(1))
    return out


if __name__ == "__main__":
    doc = {name: dict(parse(os.path.join(REF, rel)), file="Examples/" + rel) for name, rel in FILES.items()}
    json.dump(doc, open(os.path.join(ROOT, "tests", "golden", "reference_settings.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, indent=1))
    rgbd = {name: dict(parse(os.path.join(REF, rel), RGBD_KEYS), file="Examples/" + rel) for name, rel in RGBD_FILES.items()}
    json.dump(rgbd, open(RGBD_JSON, "w"), indent=1, sort_keys=True)
    print(json.dumps(rgbd, indent=1))
