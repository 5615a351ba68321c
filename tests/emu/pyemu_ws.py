"""TEST INFRASTRUCTURE ONLY: run the CPU emulation of the single-pass CSV tile
bodies for whitespace delimiters and integer label columns (emu_csv_ws.cpp,
built with AddressSanitizer) on host bytes; the result is shaped like
pyemu.parse()'s."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "_build", "emu_csv_ws_asan")

_BUILT = False


def build():
    """(Re)build the driver when its sources changed (make is a no-op otherwise)."""
    global _BUILT
    import fcntl
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    # one make at a time among parallel test workers (pyemu.build)
    with open(os.path.join(HERE, "_build", ".lock_ws"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", HERE, "-f", "csv_ws.mk"])
    _BUILT = True


def parse(data, chunk_offsets=None, index_bits=32, value_type=0, label_column=-1, weight_column=-1,
          delimiter=",", tile_bytes=0, exact=False, nthread=1):
    """CSV only.  h["path"] is "fast" when the single pass stood."""
    if not _BUILT:
        build()
    raw = data.encode("latin-1") if isinstance(data, str) else bytes(data)
    if chunk_offsets is None:
        chunk_offsets = [0, len(raw)] if raw else [0]
    with tempfile.TemporaryDirectory() as td:
        tp, cp, op = os.path.join(td, "t"), os.path.join(td, "c"), os.path.join(td, "o")
        with open(tp, "wb") as f:
            f.write(raw)
        np.asarray(chunk_offsets, dtype=np.uint64).tofile(cp)
        d = ord(delimiter) if isinstance(delimiter, str) else int(delimiter)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77")
        env.pop("EMU_EXACT", None)
        env["EMU_NTHREAD"] = str(int(nthread))
        if exact:
            env["EMU_EXACT"] = "1"
        r = subprocess.run([EXE, "1", str(index_bits), str(int(value_type)), "0", str(label_column),
                            str(weight_column), str(d), str(tile_bytes), tp, cp, op], capture_output=True, env=env)
        if r.returncode != 0:
            raise RuntimeError("emulator failed rc=%d\n%s" % (r.returncode, r.stderr.decode()[-4000:]))
        res = np.fromfile(op + ".res", dtype=np.uint64)
        it = np.uint32 if index_bits == 32 else np.uint64
        vt = {0: np.float32, 1: np.int32, 2: np.int64}[int(value_type)]
        return {
            "offset": np.fromfile(op + ".offset", dtype=np.uint64),
            "label": np.fromfile(op + ".label", dtype=vt),
            "weight": np.fromfile(op + ".weight", dtype=np.float32),
            "qid": np.fromfile(op + ".qid", dtype=np.uint64),
            "field": np.fromfile(op + ".field", dtype=it),
            "index": np.fromfile(op + ".index", dtype=it),
            "value": np.fromfile(op + ".value", dtype=vt),
            "chunk_table": np.fromfile(op + ".chunks", dtype=np.uint64).reshape(-1, 8),
            "error": int(res[8]),
            "counts": [int(x) for x in res[:8]],
            "path": "fast" if b"path=fast" in r.stderr else "exact",
        }
