#!/usr/bin/env python3
"""tests/golden/reference_optimizeessentialgraph_interface.json: the declaration adapter/essential/OptimizeEssentialGraph.cc has to define,
as names and types only -- the return type, the storage class and the parameter types of Optimizer::OptimizeEssentialGraph in the
reference's include/Optimizer.h (after tools/gen_optimizesim3_interface.py).

tests/test_eg_adapter.py compares the stand-in header the adaptor compiles against (tests/cvstub_eg/Optimizer.h) and the adaptor's own
definition with the fixture and, where the reference checkout is present, re-derives the fixture from its header and requires equality.
The reference's header is `using namespace std` through its includes and the stand-in is not: `std::` is dropped from every type.
Needs the reference checkout:  python tools/gen_optimizeessentialgraph_interface.py [reference checkout]"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_reference_fixtures as rf  # noqa: E402

FIXTURE = os.path.join(rf.GOLDEN, "reference_optimizeessentialgraph_interface.json")


def decl(text, qualified=False):
    """{"static": bool, "return": type, "params": [types]} of `OptimizeEssentialGraph(...)` in a header (or, qualified, of the definition
    `Optimizer::OptimizeEssentialGraph(...)` in a source file, where `static` is not repeated)"""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S).replace("std::", "")
    name = r"Optimizer\s*::\s*OptimizeEssentialGraph" if qualified else r"OptimizeEssentialGraph"
    m = re.search(r"([\w:\s]*?)\b" + name + r"\s*\(([^;{)]*)\)", text)
    head = m.group(1).split(":")[-1].split()     # behind an access specifier, if one stands in front
    return {"static": "static" in head, "return": " ".join(w for w in head if w != "static"),
            "params": [re.sub(r"\s+", " ", re.sub(r"\s*([<>,*&])\s*", r"\1", p)).strip() for p in rf._params(m.group(2))]}


def main(ref):
    rec = decl(open(os.path.join(ref, "include", "Optimizer.h"), errors="replace").read())
    json.dump(rec, open(FIXTURE, "w"), indent=1, sort_keys=True)
    print("wrote", os.path.relpath(FIXTURE, ROOT), os.path.getsize(FIXTURE), "bytes", rec)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(rf.gsf.REF))
