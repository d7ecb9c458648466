#!/usr/bin/env python3
"""Worst |device - truth| per front-end route, in f32 ulps of max(|truth|, 1) -- a record, not a bar (the bar is 2:
tests/test_frontend_routes.py, whose rows and checks this runs).  Prints one JSON document; profiles/frontend_routes.json keeps a run.

    python tools/frontend_routes_profile.py > profiles/frontend_routes.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import lele_amd
    import test_frontend_routes as T
    ctx = lele_amd.default_ctx(0)
    fes = T.Frontends(ctx)
    worst, rows, failed = {}, {}, []
    by_magnitude = {}   # cells under the clamp of the bar (|truth| < 1) and the others: log-mel rows of the single-utterance calls
    for row in T.ROWS:
        if not row["route"]:
            continue
        bad = T.run_row(fes, row, worst)
        rows[row["route"]] = rows.get(row["route"], 0) + 1
        failed += [(row["id"], b) for b in bad]
        if row["entry"] == "compute":
            x, _, _, _, truth = T.cases_of(row)[0]
            u = T.ulps(fes.get(row["cfg"], row["forced_regs"]).logmel(x).numpy(), truth)
            for name, sel in (("below_one", abs(truth) < 1), ("one_and_above", abs(truth) >= 1)):
                if sel.any():
                    d = by_magnitude.setdefault(name, {"cells": 0, "worst_ulps": 0.0})
                    d["cells"] += int(sel.sum())
                    d["worst_ulps"] = max(d["worst_ulps"], float(u[sel].max()))
    for row in T.BIG_ROWS:
        bad = T.run_big(fes, row, worst)
        rows[row["route"]] = rows.get(row["route"], 0) + 1
        failed += [(row["id"], b) for b in bad]
    print(json.dumps({
        "what": "MI355X: worst |device log-mel - float64 ln(max(E_oracle, 1e-5f))| per route, in ulp32(max(|truth|, 1)); bar: 2 (tests/test_frontend_routes.py)",
        "worst_ulps": {k: round(v, 3) for k, v in sorted(worst.items())},
        "rows": dict(sorted(rows.items())),
        "by_magnitude": by_magnitude,
        "failed": failed,
    }, indent=1))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
