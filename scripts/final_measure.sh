# round-end measurement batch on the GPU box: default bench with every leg (--full: per-kernel table, cpu_baseline), 1-rank
# torchrun (RCCL path, comm_ms_exposed), rocprofv3 kernel stats of the plain run, FETCH_SIZE / WRITE_SIZE passes (eager,
# separate).  usage: bash scripts/final_measure.sh OUT_DIR   (run from the repository root)
set -e
O=${1:?usage: bash scripts/final_measure.sh OUT_DIR}
mkdir -p $O
echo "[1] default bench"; timeout -k 10 500 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
echo "[2] torchrun 1 rank"; timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29517 bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline > $O/bench_torchrun1.json 2> $O/bench_torchrun1.err
echo "[3] rocprof stats"; timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o r -- python bench.py --steps 20 --warmup 5 > $O/bench_prof.json 2> $O/bench_prof.err
echo "[4] pmc fetch"; timeout -k 10 400 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -o r -- python bench.py --eager --steps 5 --warmup 2 > $O/pmc_fetch.json 2> $O/pmc_fetch.err
echo "[5] pmc write"; timeout -k 10 400 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -o r -- python bench.py --eager --steps 5 --warmup 2 > $O/pmc_write.json 2> $O/pmc_write.err
rm -f $O/*/*kernel_trace.csv $O/prof/*trace.csv
ls -la $O $O/*
