#!/bin/bash
# RDS decoding chain (k_rds_decode) measurements on an MI355X, run from the repo root: `bash tools/rds_decode_evidence.sh prof|ab OUT`.
# Outputs under OUT (kept: the rocprofv3 kernel statistics, the JSON lines and the command lines; profiles/rds_decode/ holds the committed copy).
#   1. the kernel alone, 4096 / 16384 stations, locked and hunting (tools/rds_decode_probe.py), each in a rocprofv3 run of its own
#   2. inside the pipeline: tools/bench_rds_decode.py (bench.py with the flag; random RDS bits: hunting) at 4096 and 16384 stations, and bench.py without the flag
#      (the trace must show no k_rds_decode)
#   3. bench.py and tools/bench_rds_decode.py interleaved, three times each (configs[2], primary value only)
# First argument: prof (1 + 2) or ab (3) — two runs of a few minutes each.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
PART=${1:?prof or ab}
O=$(realpath -m "${2:?output directory}")
mkdir -p $O
cd $R
Q="--no-cpu-baseline --no-other-mode --no-configs --no-host-fed"
prof() { n=$1; shift; echo "rocprofv3 --kernel-trace --stats --output-format csv -d \$OUT/$n -o run -- $*" > $O/$n.cmd
         rocprofv3 --kernel-trace --stats --output-format csv -d $O/$n -o run -- "$@" > $O/$n.json 2> $O/$n.err
         find $O/$n -name '*kernel_stats.csv' -exec cp {} $O/${n}_kernel_stats.csv \; ; rm -rf $O/$n; }
if [ "$PART" = prof ]; then
for C in 4096 16384; do
  for S in locked hunting; do prof probe_${S}_$C python3 tools/rds_decode_probe.py --channels $C --state $S --launches 200; done
done
prof bench_rds_4096 python3 tools/bench_rds_decode.py --steps 50 --warmup 3 $Q
prof bench_rds_16384 python3 tools/bench_rds_decode.py --channels 16384 --steps 50 --warmup 3 $Q
prof bench_noflag_4096 python3 bench.py --steps 50 --warmup 3 $Q
fi
if [ "$PART" = ab ]; then
for i in 1 2 3; do
  python3 bench.py $Q > $O/ab_default_$i.json 2> /dev/null
  python3 tools/bench_rds_decode.py $Q > $O/ab_rds_$i.json 2> /dev/null
done
echo "python3 bench.py $Q  /  python3 tools/bench_rds_decode.py $Q, interleaved x3" > $O/ab.cmd
fi
ls -la $O
