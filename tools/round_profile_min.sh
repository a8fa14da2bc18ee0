#!/bin/bash
# A SHORT session for a library change that touches one kernel family late in a round (the full one: tools/round_profile.sh):
# the tests of that family, the kernel trace + FETCH_SIZE / WRITE_SIZE passes of every bench row (profiles/pmc_traffic.json is
# keyed by the library hash, so all rows are taken again), the bench line.
#   tools/round_profile_min.sh r04h "gru or wavefront or reserve or captur or posteriors_only"
set -u
tag=${1:-r04h}
sel=${2:-gru}
root=${GRAFT_REPO_ROOT:-$PWD}
out=$root/gpurun_out
mkdir -p $out
cd $root
python -m pytest tests -m gpu -q -k "$sel" 2>&1 | tail -3 > $out/${tag}_pytest_gpu_subset.txt
tools/pmc_min.sh hl python bench.py --no-cpu-baseline --no-extras --steps 7 --warmup 2 > /dev/null
tools/pmc_min.sh hl32 python bench.py --no-cpu-baseline --no-extras --steps 7 --warmup 2 --precision f32 > /dev/null
tools/pmc_min.sh md python bench.py --model mdtc_h64 --no-cpu-baseline --no-extras --steps 7 --warmup 2 > /dev/null
tools/pmc_min.sh gru python bench.py --model gru_2x128 --no-cpu-baseline --no-extras --steps 7 --warmup 2 > /dev/null
tools/pmc_min.sh d64 python bench.py --model ds_tcn_h64 --no-cpu-baseline --no-extras --steps 7 --warmup 2 > /dev/null
tools/pmc_min.sh m32 python bench.py --model mdtc_small --no-cpu-baseline --no-extras --steps 7 --warmup 2 > /dev/null
python tools/prof_summary.py $(find $out -path "*prof_*" -name "*_results.db" | sort) > $out/${tag}_traffic_passes.txt
p=profiles/${tag}_traffic_passes.txt
python tools/pmc_traffic.py ds_tcn_h256/B1024/f16x3=hl=$p ds_tcn_h256/B1024/f32=hl32=$p mdtc_h64/B1024/f16x3=md=$p gru_2x128/B1024/f16x3=gru=$p ds_tcn_h64/B1024/f16x3=d64=$p mdtc_small/B1024/f16x3=m32=$p > $out/${tag}_pmc_traffic.log 2>&1
cp profiles/pmc_traffic.json $out/${tag}_pmc_traffic.json
rm -rf $out/prof_*
python bench.py --full --extras-out $out/${tag}_bench_extras.json 2> $out/${tag}_bench.err | tail -1 > $out/${tag}_bench.json
