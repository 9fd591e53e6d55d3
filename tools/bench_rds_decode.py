#!/usr/bin/env python3
"""bench.py with the RDS decoding chain on the timed handle (FMD_FLAG_RDS_DECODE): the cost of the decoder beside the demodulator.

bench.py is the project's yardstick and stays as it is; this runs it in-process with the package's BatchDemod built with rds_decode=True
and marks its JSON line ("rds_decode": true).  Every handle bench.py creates gets the flag, so pass --no-other-mode --no-configs (the
side lines would decode too) and keep --gpus 1.  bench.py's synthetic RDS is random bits: the decoder stays in its hunting path.

    python tools/bench_rds_decode.py --no-cpu-baseline --no-other-mode --no-configs --no-host-fed
"""
import contextlib
import io
import json
import runpy
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> None:
    if "--gpus" in sys.argv and sys.argv[sys.argv.index("--gpus") + 1] != "1":
        raise SystemExit("bench_rds_decode.py: --gpus 1 only")
    import fmradio_loader
    pkg = fmradio_loader.load()
    base = pkg.BatchDemod

    class BatchDemodWithDecode(base):
        def __init__(self, *args, **kw):
            kw.setdefault("rds_decode", True)
            super().__init__(*args, **kw)

    pkg.BatchDemod = BatchDemodWithDecode
    sys.argv = [str(ROOT / "bench.py")] + sys.argv[1:]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        runpy.run_path(str(ROOT / "bench.py"), run_name="__main__")
    lines = out.getvalue().splitlines()
    for i in range(len(lines) - 1, -1, -1):          # the result line is the last JSON object bench.py prints
        if lines[i].startswith("{") and '"metric"' in lines[i]:
            d = json.loads(lines[i])
            d["rds_decode"] = True
            d["config"]["rds_decode"] = True
            lines[i] = json.dumps(d)
            break
    print("\n".join(lines))


if __name__ == "__main__":
    main()
