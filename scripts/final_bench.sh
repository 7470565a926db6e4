set -o pipefail
R=${RESULTS_DIR:-results}        # output directory, relative to the repository root
cd $GRAFT_REPO_ROOT
mkdir -p $R/final
timeout -k 10 1000 python -m pytest tests -m gpu -x -q > $R/final/tests.log 2>&1; echo "tests rc=$?" ; tail -2 $R/final/tests.log
python bench.py --full --steps 20 --warmup 5 > $R/final/default.json 2> $R/final/default.err; echo "default rc=$?"
python bench.py --full --steps 20 --warmup 5 --gemm bf16 --no-cpu-baseline > $R/final/bf16.json 2> $R/final/bf16.err; echo "bf16 rc=$?"
python bench.py --full --batch 32 --points 2048 --steps 50 --warmup 10 --no-cpu-baseline > $R/final/b32.json 2>/dev/null
python bench.py --full --batch 32 --points 2048 --steps 50 --warmup 10 --no-cpu-baseline --graph > $R/final/b32g.json 2>/dev/null
python bench.py --full --batch 512 --points 2048 --steps 10 --warmup 3 --no-cpu-baseline > $R/final/b512.json 2>/dev/null
python bench.py --full --batch 512 --points 2048 --steps 10 --warmup 3 --no-cpu-baseline --gemm bf16 > $R/final/b512_bf16.json 2>/dev/null
python bench.py --full --batch 4096 --points 2048 --steps 5 --warmup 2 --no-cpu-baseline --gemm bf16 > $R/final/b4096n2048_bf16.json 2>/dev/null
for f in default bf16 b32 b32g b512 b512_bf16 b4096n2048_bf16; do echo $f; cut -c90-260 $R/final/$f.json; done
