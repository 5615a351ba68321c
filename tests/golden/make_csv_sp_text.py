#!/usr/bin/env python3
"""Generate tests/golden/csv_sp_text.json from the GENUINE reference
(oracle/_ref/libdmlc_ref.so): float CSV with label_column / weight_column over
header rows, text, missing values, blanks and BOMs.

    make -C oracle ref && python tests/golden/make_csv_sp_text.py

Data only, in the layout of csv_ws.json: the inputs (tests/fuzz_csv_sp.py
table(), the small edge_cases() and violations()), the chunk offsets and the
arrays the reference's ParseBlock produced.
"""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fuzz_csv_sp as fz  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MAX_BYTES = 400  # per input: the fixture stays a few tens of KB


def enc(a):
    a = np.asarray(a)
    if a.dtype == np.float32:
        return {"dtype": "f32bits", "data": a.view(np.uint32).tolist()}
    return {"dtype": str(a.dtype), "data": a.tolist()}


def message(msg):
    """The reference's error text alone: "<file>:<line>: <message>", without the
    time stamp, the build's directories and the stack trace."""
    msg = msg.split("\nStack trace", 1)[0].strip()
    return re.sub(r"^\[[0-9:]+\] \S*/", "", msg)


def inputs():
    for name, text, lc, wc, fast in fz.table():
        yield "table_" + name, text.encode("latin-1"), lc, wc, ",", bool(fast)
    for name, data, lc, wc, delim, fast in fz.edge_cases():
        if len(data) <= MAX_BYTES:
            yield "edge_" + name, data, lc, wc, delim, bool(fast)
    for name, text, lc, wc in fz.violations():
        yield "viol_" + name, text.encode("latin-1"), lc, wc, ",", False


def main():
    if not po.ref_available():
        sys.exit("build the reference first: make -C oracle ref")
    out = []
    for name, data, lc, wc, delim, fast in inputs():
        offs = [0, len(data)]
        kw = {"fmt": po.CSV, "delimiter": delim, "value_kind": po.F32, "label_column": lc, "weight_column": wc}
        r = po.ref_parse_chunks(data, offs, **kw)
        rec = {"name": name, "data_latin1": data.decode("latin-1"), "offs": offs, "params": kw, "fast": fast,
               "exact": name.startswith("viol_"), "status": int(r["status"] != 0), "msg": message(r["msg"])}
        if r["status"] == 0:
            rec["expect"] = {k: enc(r[k]) for k in ("offset", "label", "weight", "qid", "field", "index", "value")}
        out.append(rec)
    with open(os.path.join(OUT, "csv_sp_text.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in out) + "\n]\n")  # one case per line
    print("csv_sp_text.json:", len(out), "cases,", sum(r["status"] for r in out), "error cases")


if __name__ == "__main__":
    main()
