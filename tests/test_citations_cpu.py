"""Every `<reference file>.py:<line>[-<line>]` citation in the boundary header
and the design notes points inside the cited reference file.  The reference's
line counts are a stored fixture (tests/golden/reference_line_counts.json,
written by tests/golden/gen_golden.py line_counts), so the reference tree itself
is not needed."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")
DOCS = ("include/rx.h", "DESIGN.md", "INTEGRATION.md")


def _ref_files():
    """Line counts by relative path, and by bare file name (every file of that name)."""
    out = {}
    for rel, n in json.load(open(COUNTS)).items():
        out.setdefault(os.path.basename(rel), []).append(n)
        out[rel] = [n]
    return out


@pytest.mark.parametrize("doc", DOCS)
def test_citations_point_inside_the_reference(doc):
    files = _ref_files()
    text = open(os.path.join(ROOT, doc)).read()
    bad = []
    for m in re.finditer(r"([\w/]+\.py):(\d+(?:-\d+)?(?:,\d+(?:-\d+)?)*)", text):
        name, spans = m.group(1), m.group(2)
        cands = files.get(name) if "/" in name else files.get(name)
        if not cands:
            continue  # not a reference file (this repo's own modules)
        n = max(cands)
        for span in spans.split(","):
            hi = int(span.split("-")[-1])
            if hi > n:
                bad.append(f"{m.group(0)} (file has {n} lines)")
    assert not bad, bad
