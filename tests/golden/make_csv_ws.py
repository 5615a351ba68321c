#!/usr/bin/env python3
"""Generate tests/golden/csv_ws.json from the GENUINE reference
(oracle/_ref/libdmlc_ref.so): CSV with ' ' and '\\t' as the delimiter.

    make -C oracle ref && python tests/golden/make_csv_ws.py

Data only, in the layout of filldata.json: the inputs (tests/fuzz_ws.py table(),
the small edge_cases() and violations()), the chunk offsets and the arrays the
reference's ParseBlock produced, for float and int32 values.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fuzz_ws  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MAX_BYTES = 400  # per input: the fixture stays a few tens of KB


def enc(a):
    a = np.asarray(a)
    if a.dtype == np.float32:
        return {"dtype": "f32bits", "data": a.view(np.uint32).tolist()}
    return {"dtype": str(a.dtype), "data": a.tolist()}


def inputs():
    for delim, dn in (("\t", "tab"), (" ", "space")):
        for name, text, fast in fuzz_ws.table(delim):
            yield "table_%s_%s" % (name, dn), text.encode("latin-1"), None, delim, fast, name == "text_fields"
        for name, data, offs, fast, f32_only in fuzz_ws.edge_cases(delim):
            keep = name.startswith(("seg_", "run62_at63", "run62_at64", "run64_", "run130_", "cut_", "crlf", "header", "junk"))
            if keep and len(data) <= MAX_BYTES and offs is not None:
                yield "edge_%s_%s" % (name, dn), data, None if offs == "whole" else offs, delim, fast, f32_only
        for name, data, offs in fuzz_ws.violations(delim):
            yield "viol_%s_%s" % (name, dn), data, offs, delim, False, False


def main():
    if not po.ref_available():
        sys.exit("build the reference first: make -C oracle ref")
    out = []
    for name, data, offs, delim, fast, f32_only in inputs():
        offs = [int(x) for x in (offs if offs is not None else ([0, len(data)] if data else [0]))]
        for vk, vn in ((po.F32, "f32"), (po.I32, "i32")):
            kw = {"fmt": po.CSV, "delimiter": delim, "value_kind": vk}
            r = po.ref_parse_chunks(data, offs, **kw)
            rec = {"name": "%s_%s" % (name, vn), "data_latin1": data.decode("latin-1"), "offs": offs, "params": kw,
                   "fast": bool(fast and not (f32_only and vk != po.F32)), "status": int(r["status"] != 0),
                   "msg": r["msg"]}
            if r["status"] == 0:
                rec["expect"] = {k: enc(r[k]) for k in ("offset", "label", "weight", "qid", "field", "index", "value")}
            out.append(rec)
    with open(os.path.join(OUT, "csv_ws.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in out) + "\n]\n")  # one case per line
    print("csv_ws.json:", len(out), "cases,", sum(r["status"] for r in out), "error cases")


if __name__ == "__main__":
    main()
