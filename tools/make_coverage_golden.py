#!/usr/bin/env python3
"""Record the coverage block of a TLC -tool run (MC.out) as a test fixture.

    python tools/make_coverage_golden.py <MC.out> [out.json]

Writes tests/golden/model1_coverage.json: the ordered list of every
2773/2772/2221/2775/2774 message between 2201 ("The coverage statistics") and
2202 ("End of statistics") as

    {code, depth, span, name, count, cost, mcout_line}

depth is the number of '|' in front of the span (TLC's nesting), span is
[line, col, line, col] in KubeAPI.tla, name is the definition's name on the
2773/2772/2774 headers (None otherwise), count is the evaluation count (the
generated count of a header; None on a 2774), cost the second number of a 2775
line or the distinct count of a 2773/2772 header (None otherwise), and
mcout_line the 1-based line of MC.out that holds the message body.  These are
recorded results only; the tests read this file, never the run it came from.
"""
from __future__ import annotations

import json
import os
import re
import sys

CODES = (2773, 2772, 2221, 2775, 2774)
SPAN = r"line (\d+), col (\d+) to line (\d+), col (\d+) of module KubeAPI"
HEAD = re.compile(r"^<(\w+) " + SPAN + r">(?:: (\d+):(\d+))?$")
EXPR = re.compile(r"^  (\|*)" + SPAN + r": (\d+)(?::(\d+))?$")


def parse(text: str) -> list:
    lines = text.splitlines()
    out, inside = [], False
    for i, ln in enumerate(lines):
        m = re.match(r"^@!@!@STARTMSG (\d+):\d+ @!@!@$", ln)
        if not m:
            continue
        code = int(m.group(1))
        if code == 2201:
            inside, out = True, []      # the last (final) coverage block wins
            continue
        if code == 2202:
            inside = False
            continue
        if not inside or code not in CODES:
            continue
        body = lines[i + 1]
        if code in (2773, 2772, 2774):
            h = HEAD.match(body)
            if not h:
                raise ValueError(f"line {i + 2}: {body!r}")
            dist, gen = h.group(6), h.group(7)
            out.append({"code": code, "depth": 0, "span": [int(h.group(k)) for k in (2, 3, 4, 5)],
                        "name": h.group(1), "count": int(gen) if gen else None,
                        "cost": int(dist) if dist else None, "mcout_line": i + 2})
        else:
            e = EXPR.match(body)
            if not e:
                raise ValueError(f"line {i + 2}: {body!r}")
            out.append({"code": code, "depth": len(e.group(1)), "span": [int(e.group(k)) for k in (2, 3, 4, 5)],
                        "name": None, "count": int(e.group(6)),
                        "cost": int(e.group(7)) if e.group(7) else None, "mcout_line": i + 2})
    return out


def main(argv) -> int:
    if len(argv) < 2:
        print(__doc__, file=sys.stderr)
        return 2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dst = argv[2] if len(argv) > 2 else os.path.join(root, "tests", "golden", "model1_coverage.json")
    entries = parse(open(argv[1]).read())
    with open(dst, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")
    by = {c: sum(1 for e in entries if e["code"] == c) for c in CODES}
    print(f"{dst}: {len(entries)} entries {by}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
