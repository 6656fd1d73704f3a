#!/usr/bin/env python3
"""Data fixtures that let the tests pinning this project to the REFERENCE run without its checkout.

Each is extracted from the reference's text into tests/golden/; the tests always compare against the fixture and, where
the reference checkout is present, re-derive the fixture from the text with the same parsers here and require equality:

  reference_orbmatcher_signatures.json  parameter types of the ORBmatcher searches the adaptor defines (include/ORBmatcher.h)
  reference_dbow2_interface.json        typedefs, base classes and FeatureVector::addFeature of Thirdparty/DBoW2/DBoW2/{BowVector,FeatureVector}.h
  reference_bit_pattern_31.npy          the 1024 values of bit_pattern_31_ (src/ORBextractor.cc:160-418) as int8, interleaved x0,y0,x1,y1
  reference_settings_lines.json         the `key: value` lines of Examples/*/*.yaml that tests/golden/reference_settings.json holds

(the DBoW2 accumulation vectors come from tools/gen_dbow2_golden.py, which needs oracle/_ref).
Needs the reference checkout:  python tools/gen_reference_fixtures.py [reference checkout]"""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_settings_fixture as gsf  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ORBMATCHER_NAMES = ("SearchByProjection", "SearchByBoW", "SearchForInitialization", "SearchForTriangulation", "SearchBySim3", "Fuse")
SIGNATURES = os.path.join(GOLDEN, "reference_orbmatcher_signatures.json")
DBOW2_INTERFACE = os.path.join(GOLDEN, "reference_dbow2_interface.json")
PATTERN = os.path.join(GOLDEN, "reference_bit_pattern_31.npy")
SETTINGS_LINES = os.path.join(GOLDEN, "reference_settings_lines.json")


def _params(text):
    """normalised parameter types of a C++ parameter list (default values and parameter names dropped)"""
    params = []
    for prm in text.split(","):
        prm = re.sub(r"=[^,]*$", "", prm)                      # default value
        prm = re.sub(r"\bstd::", "", prm)
        prm = re.sub(r"\s*([*&<>])\s*", r"\1", " ".join(prm.split()))
        prm = re.sub(r"[*&]?\s*\w+$", lambda t: t.group(0)[0] if t.group(0)[0] in "*&" else "", prm).strip()   # drop the parameter name
        params.append(prm)
    return params


def orbmatcher_decls(text, names=ORBMATCHER_NAMES):
    """{method name: [normalised parameter lists]} of the member declarations `int name(...);` in a header"""
    out = {}
    for m in re.finditer(r"\bint\s+(\w+)\s*\(([^;{]*)\)\s*;", text):
        if m.group(1) in names:
            out.setdefault(m.group(1), []).append(tuple(_params(m.group(2))))
    return out


def _type(s):
    return re.sub(r"\s*([<>,])\s*", r"\1", " ".join(s.split()))


def dbow2_interface(dbow2_dir):
    """what the adaptor relies on of DBoW2: the id / value typedefs, the std::map bases of BowVector and FeatureVector, and
    FeatureVector::addFeature's parameter types, from BowVector.h + FeatureVector.h in `dbow2_dir`"""
    text = ""
    for f in ("BowVector.h", "FeatureVector.h"):
        text += re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(dbow2_dir, f), errors="replace").read(), flags=re.S) + "\n"
    typedefs = {n: _type(t) for t, n in re.findall(r"\btypedef\s+([\w\s:<>,]+?)\s+(\w+)\s*;", text) if n in ("WordId", "WordValue", "NodeId")}
    bases = {n: _type(b) for n, b in re.findall(r"\bclass\s+(BowVector|FeatureVector)\s*:\s*public\s+(std::map<.*?>)\s*\{", text, re.S)}
    m = re.search(r"\bvoid\s+addFeature\s*\(([^)]*)\)", text)
    return {"typedefs": typedefs, "bases": bases, "FeatureVector::addFeature": _params(m.group(1)) if m else None}


def pattern_values(text):
    """the int8[1024] bit_pattern_31_ table of the reference's src/ORBextractor.cc, in its own order"""
    m = re.search(r"bit_pattern_31_\[256\*4\]\s*=\s*\{(.*?)\};", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return np.array([int(t) for t in re.findall(r"-?\d+", body)], np.int8)


def settings_lines(text):
    """the `key: value` lines of a settings file that gen_settings_fixture.parse reads, stripped, in KEYS order"""
    out = []
    for k in gsf.KEYS:
        m = re.search(r"^%s\s*:\s*[-+0-9.eE]+" % re.escape(k), text, re.M)
        if m:
            out.append(m.group(0).strip())
    return out


def main(ref):
    sig = orbmatcher_decls(open(os.path.join(ref, "include", "ORBmatcher.h"), errors="replace").read())
    json.dump({k: [list(s) for s in v] for k, v in sorted(sig.items())}, open(SIGNATURES, "w"), indent=1)
    json.dump(dbow2_interface(os.path.join(ref, "Thirdparty", "DBoW2", "DBoW2")), open(DBOW2_INTERFACE, "w"), indent=1)
    vals = pattern_values(open(os.path.join(ref, "src", "ORBextractor.cc"), encoding="utf-8", errors="replace").read())
    assert len(vals) == 1024
    np.save(PATTERN, vals)
    lines = {name: settings_lines(open(os.path.join(ref, "Examples", rel), encoding="utf-8", errors="replace").read()) for name, rel in gsf.FILES.items()}
    json.dump(lines, open(SETTINGS_LINES, "w"), indent=1, sort_keys=True)
    for p in (SIGNATURES, DBOW2_INTERFACE, PATTERN, SETTINGS_LINES):
        print("wrote", os.path.relpath(p, ROOT), os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(gsf.REF))
