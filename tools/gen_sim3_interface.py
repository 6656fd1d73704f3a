#!/usr/bin/env python3
"""tests/golden/reference_sim3solver_interface.json: what adapter/sim3/Sim3Solver.h has to meet and what the contract of include/orbx.h
rests on, as names and types only --

  public       return type and parameter types of every public member of the reference's include/Sim3Solver.h, in declaration order
  max_error    the declared element type of mvnMaxError1 / mvnMaxError2 (size_t: the thresholds are truncated)

tests/test_sim3_adapter.py compares the adaptor's header against the fixture and, where the reference checkout is present, re-derives the
fixture from its header with the parser here and requires equality (as tools/gen_reference_fixtures.py does for ORBmatcher.h).
Needs the reference checkout:  python tools/gen_sim3_interface.py [reference checkout]"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import gen_reference_fixtures as rf  # noqa: E402

FIXTURE = os.path.join(rf.GOLDEN, "reference_sim3solver_interface.json")


def sim3solver_interface(text):
    """{"public": [[name, return type, [parameter types]], ...], "max_error": {member: element type}} of a Sim3Solver header"""
    text = re.sub(r"#ifdef ORBX_ADAPTER_CAPTURE.*?#endif", "", text, flags=re.S)      # the adaptor's test hook is not interface
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)
    body = text[re.search(r"\bclass\s+Sim3Solver\s*\{", text).end():]
    public = body[body.index("public:") + 7:]
    public = public[:re.search(r"\b(protected|private)\s*:", public).start()]
    decls = []
    for m in re.finditer(r"([\w:<>*&\s]*?)\b(\w+)\s*\(([^;{]*)\)\s*;", public):
        ret = re.sub(r"\bstd::", "", " ".join(m.group(1).split()))
        decls.append([m.group(2), ret, rf._params(m.group(3)) if m.group(3).strip() else []])
    elem = {n: re.sub(r"\bstd::", "", t).strip() for t, n in re.findall(r"\bstd::vector<\s*([\w:\s]+?)\s*>\s+(mvnMaxError[12])\s*;", body)}
    return {"public": decls, "max_error": elem}


def main(ref):
    rec = sim3solver_interface(open(os.path.join(ref, "include", "Sim3Solver.h"), errors="replace").read())
    json.dump(rec, open(FIXTURE, "w"), indent=1, sort_keys=True)
    print("wrote", os.path.relpath(FIXTURE, ROOT), os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(rf.gsf.REF))
