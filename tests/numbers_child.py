"""TEST INFRASTRUCTURE ONLY -- child process of test_gpu_numbers.py's lean-kernel test.

Sets DMLC_AMD_LEAN=1 before the PRODUCT library loads (as tests/lean_child.py),
so libsvm full calls launch svm_lean_tile, and runs the number catalogue's
libsvm inputs through it: the dense value-role input and the compact roles
(tests/numcases.py), and the clustered many-chunks input of
tests/lean_child.py, which stays on the single pass only when the lean kernel
ran.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["DMLC_AMD_LEAN"] = "1"
os.environ.pop("DMLC_AMD_LIB", None)  # the product library, not a variant
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "dmlc-core_amd", "python")]

import dmlc_amd  # noqa: E402
import full_call as fc  # noqa: E402
import numcases as nc  # noqa: E402
from oracle import pyoracle as po  # noqa: E402


def main():
    cases = [c for c in nc.dense_cases() + nc.role_cases() if c["fmt"] == po.LIBSVM]
    out = {"cases": []}
    for c in cases:
        e = {k: c[k] for k in ("name", "expect", "parsed", "numbers", "window", "byte")}
        try:
            h = nc.run_case(dmlc_amd, fc, c)
            e.update(ok=True, path=h["path"], error=h["error"], status=h["oracle"]["status"])
        except AssertionError as ex:
            e.update(ok=False, msg=str(ex)[:800], path=-1, status=-1)
        out["cases"].append(e)
    data, offs = fc.cluster_chunks(*dmlc_amd.fast_geometry())
    try:
        out["cluster_path"] = fc.full_vs_oracle(dmlc_amd, data, offs, po.LIBSVM)["path"]
    except AssertionError as ex:
        out["cluster_path"] = str(ex)[:600]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
