#!/bin/bash
# SQ counters of nlr_resample_kernel alone (scripts/resample_ab.py, 11 dispatches per launch shape and input), two --pmc passes, no
# tracing domains.  usage: [NLR_LIB_PATH=<lib>] [PMC_OUT=<dir>] scripts/pmc_resample.sh TAG     prints one line per pass, input and launch shape
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-build}
OUT=${PMC_OUT:-$ROOT/out/pmc_resample}/$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_WAIT_ANY --output-format csv -d $OUT/p1 -- python3 $ROOT/scripts/resample_ab.py $TAG --launches 10 > $OUT/p1.log 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_LDS_IDX_ACTIVE SQ_INSTS_SALU SQ_ACTIVE_INST_SCA --output-format csv -d $OUT/p2 -- python3 $ROOT/scripts/resample_ab.py $TAG --launches 10 > $OUT/p2.log 2>&1 || exit 1
cd $ROOT
grep '^#' $OUT/p1.log
python3 - $OUT $TAG <<'PY'
import csv, glob, collections, sys
out, tag = sys.argv[1:3]
shapes = ["noise 0->64", "noise 64->64", "noise 64->128", "peak 0->64", "peak 64->64", "peak 64->128"]
for d in ("p1", "p2"):
    for f in glob.glob(f"{out}/{d}/**/*counter_collection.csv", recursive=True):
        per = collections.defaultdict(dict)          # dispatch id -> counter -> value
        for r in csv.DictReader(open(f)):
            if "nlr_resample_kernel" in r["Kernel_Name"]:
                per[int(r["Dispatch_Id"])][r["Counter_Name"]] = per[int(r["Dispatch_Id"])].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
        ids = sorted(per)
        assert len(ids) == 11 * len(shapes), len(ids)
        for i, name in enumerate(shapes):            # dispatches in launch order: 1 warm-up + 10 per shape; the mean of the 10
            rows = [per[j] for j in ids[11 * i + 1: 11 * (i + 1)]]
            print(tag, d, f"{name:13s}", {c: f"{sum(r[c] for r in rows) / len(rows):.4g}" for c in rows[0]})
PY
