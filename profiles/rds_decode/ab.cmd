python3 bench.py --no-cpu-baseline --no-other-mode --no-configs --no-host-fed  /  python3 tools/bench_rds_decode.py --no-cpu-baseline --no-other-mode --no-configs --no-host-fed, interleaved x3
