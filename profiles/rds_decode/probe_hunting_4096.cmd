rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/probe_hunting_4096 -o run -- python3 tools/rds_decode_probe.py --channels 4096 --state hunting --launches 200
