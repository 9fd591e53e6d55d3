rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/bench_noflag_4096 -o run -- python3 bench.py --steps 50 --warmup 3 --no-cpu-baseline --no-other-mode --no-configs --no-host-fed
