# Multi-rank rehearsal on a one-GPU box: two ranks on cuda:0 over gloo, the real kernels,
# config 4 at 20 M objects (--full); the line lands in DIR/s2u/ (DIR: first argument, default out).
cd ${GRAFT_REPO_ROOT:-.}
O=${1:-out}/s2u
mkdir -p $O
HDX_BENCH_BACKEND=gloo timeout -k 10 500 python -u bench.py --full --gpus 2 --config4-objects 20000000 > $O/bench_gloo2.log 2> $O/bench_gloo2.err
