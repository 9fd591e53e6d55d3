rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/probe_locked_16384 -o run -- python3 tools/rds_decode_probe.py --channels 16384 --state locked --launches 200
