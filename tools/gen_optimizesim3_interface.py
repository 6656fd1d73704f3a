#!/usr/bin/env python3
"""tests/golden/reference_optimizesim3_interface.json: the declaration adapter/sim3opt/OptimizeSim3.cc has to define, as names and types
only -- the return type, the storage class and the parameter types of Optimizer::OptimizeSim3 in the reference's include/Optimizer.h.

tests/test_sim3opt_adapter.py compares the stand-in header the adaptor compiles against (tests/cvstub_sim3opt/Optimizer.h) and the
adaptor's own definition with the fixture and, where the reference checkout is present, re-derives the fixture from its header with the
parser here and requires equality (as tools/gen_sim3_interface.py does for Sim3Solver.h).
Needs the reference checkout:  python tools/gen_optimizesim3_interface.py [reference checkout]"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_reference_fixtures as rf  # noqa: E402

FIXTURE = os.path.join(rf.GOLDEN, "reference_optimizesim3_interface.json")


def optimizesim3_decl(text, qualified=False):
    """{"static": bool, "return": type, "params": [types]} of `OptimizeSim3(...)` in a header (or, qualified, of the definition
    `Optimizer::OptimizeSim3(...)` in a source file, where `static` is not repeated)"""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)
    name = r"Optimizer\s*::\s*OptimizeSim3" if qualified else r"OptimizeSim3"
    m = re.search(r"([\w:\s]*?)\b" + name + r"\s*\(([^;{)]*)\)", text)
    head = m.group(1).split(":")[-1].split()     # behind an access specifier, if one stands in front
    return {"static": "static" in head, "return": " ".join(w for w in head if w != "static"), "params": rf._params(m.group(2))}


def main(ref):
    rec = optimizesim3_decl(open(os.path.join(ref, "include", "Optimizer.h"), errors="replace").read())
    json.dump(rec, open(FIXTURE, "w"), indent=1, sort_keys=True)
    print("wrote", os.path.relpath(FIXTURE, ROOT), os.path.getsize(FIXTURE), "bytes", rec)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(rf.gsf.REF))
