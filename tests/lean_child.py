"""TEST INFRASTRUCTURE ONLY -- child process of test_gpu_full_call.py's lean-kernel test.

Sets DMLC_AMD_LEAN=1 before the PRODUCT library loads (libsvm.hip reads it
once), so a libsvm full call launches svm_lean_tile ahead of svm_fast_tile<2>,
which resumes at the first tile the lean kernel poisoned.  Runs the inputs of
full_call.lean_cases through full calls against the oracle (guard bands
included) and the clustered many-chunks input, which only the lean kernel
keeps on the single pass.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["DMLC_AMD_LEAN"] = "1"
os.environ.pop("DMLC_AMD_LIB", None)  # the product library, not a variant
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "dmlc-core_amd", "python")]

import dmlc_amd  # noqa: E402
import full_call as fc  # noqa: E402
from oracle import pyoracle as po  # noqa: E402


def main():
    tile, max_cs = dmlc_amd.fast_geometry()
    out = {"cases": []}
    for c in fc.lean_cases(tile):
        e = {"name": c["name"], "expect": c["expect"], "parsed": c["parsed"], "ok": True}
        try:
            for slack in (0, 1000):
                h = fc.full_vs_oracle(dmlc_amd, c["data"], c["offs"], po.LIBSVM, slack=slack, **c["kw"])
            e.update(path=h["path"], error=h["error"], status=h["oracle"]["status"])
        except AssertionError as ex:
            e.update(ok=False, msg=str(ex)[:600], path=-1, status=-1)
        out["cases"].append(e)
    data, offs = fc.cluster_chunks(tile, max_cs)
    try:
        out["cluster_path"] = fc.full_vs_oracle(dmlc_amd, data, offs, po.LIBSVM)["path"]
    except AssertionError as ex:
        out["cluster_path"] = str(ex)[:600]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
