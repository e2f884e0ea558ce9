#!/bin/bash
# End-of-round measurements (GPU box): kernel traces of the hot path and the training steps, per-kernel tables of the three
# registry models, the full bench line (--full) with the driver's arguments and with the defaults, the five-rank rehearsal
# on one GPU.
#     bash tools/final_measurements.sh <round> <out-dir>
# Results land under <out-dir>/<round>/; the traces of tools/profile_round.sh land where that script writes them.
RND=${1:-r06}
OUT=${2:?usage: tools/final_measurements.sh <round> <out-dir>}; O=$OUT/$RND
mkdir -p $O
bash tools/profile_round.sh $RND "hot full" > $OUT/profile_round_${RND}b.log 2>&1
python3 tools/train_kernels.py --R 3 --top 60 > $O/train_kernels_stacked_final.txt 2>/dev/null
python3 tools/train_kernels.py --R 3 --hidden 48 --top 30 > $O/train_kernels_msgat48.txt 2>/dev/null
python3 tools/train_kernels.py --R 3 --hidden 96 --top 30 > $O/train_kernels_msgat96.txt 2>/dev/null
python3 tools/train_kernels.py --R 3 --ops --top 0 2>/dev/null | grep -E "aten::|torch operators" > $O/train_step_torch_ops.txt
python3 tools/host_overhead_train.py --small > $O/host_overhead_train_small.txt 2>&1
python3 tools/causal_conv_time.py > $O/causal_conv_cold.txt 2>&1
python bench.py --full --steps 20 --warmup 5 > $O/bench_driver_args.json 2> $O/bench_driver_args.err
python bench.py --full > $O/bench_plain.json 2> $O/bench_plain.err
MSGAT_BENCH_SHARE_GPU=1 timeout -k 10 400 python bench.py --gpus 5 --steps 10 --warmup 3 --full > $O/bench_share_gpu_5ranks.json 2> $O/bench_share_gpu_5ranks.err
O=$O python - <<PY
import json, os
O = os.environ["O"]
for f in ("bench_driver_args","bench_plain","bench_share_gpu_5ranks"):
    try:
        d=json.load(open(f"{O}/{f}.json"))
        print(f, d["n_gpus"], d["ms_per_step"], d["ms_per_step_median_hip_events"], d["roofline"]["frac"], d.get("full_step_cfg3",{}).get("ms_per_step"), d.get("full_step_cfg3",{}).get("ms_per_step_median_hip_events"), d.get("full_step_cfg4",{}).get("ms_per_step"), d.get("allreduce_us"))
    except Exception as e:
        print(f, "ERR", e)
PY
