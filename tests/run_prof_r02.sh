set -e
R=$(pwd)
mkdir -p prof_out/r02
timeout -k 10 400 python bench.py --full > prof_out/r02/bench_c3.json 2> prof_out/r02/bench_c3.err
timeout -k 10 200 python bench.py --full --workload c4 --no-cpu-baseline > prof_out/r02/bench_c4.json 2> prof_out/r02/bench_c4.err
cd /tmp && export TMPDIR=/tmp && export MI_PHYSICS_NO_GRAPH=1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/prof_out/r02/stats -o c3 -- python3 $R/bench.py --full --steps 100 --no-cpu-baseline > $R/prof_out/r02/stats.log 2>&1
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $R/prof_out/r02/pmc_fetch -o c3 -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $R/prof_out/r02/pmc_fetch.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $R/prof_out/r02/pmc_write -o c3 -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $R/prof_out/r02/pmc_write.log 2>&1
cd $R; ls -la prof_out/r02/*; cat prof_out/r02/bench_c3.json prof_out/r02/bench_c4.json
