rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/probe_hunting_16384 -o run -- python3 tools/rds_decode_probe.py --channels 16384 --state hunting --launches 200
