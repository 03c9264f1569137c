set -o pipefail
# usage (repo root): OUT=<results directory, default results/> bash profiles/gpu_suite.sh
OUT=${OUT:-results}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/r03a_pytest.log 2>&1 && \
timeout -k 10 600 python -u bench.py --full > $OUT/r03a_bench.json 2> $OUT/r03a_bench.err
