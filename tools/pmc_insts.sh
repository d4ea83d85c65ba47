set -e
# GPU suite, one bench line with per-kernel times, then SQ counter passes of the bench workload (one rocprofv3 --pmc run
# per counter group).  usage: tools/pmc_insts.sh <output dir>   (relative paths: from the repository root)
cd "$(dirname "$0")/.."
O=${1:?usage: tools/pmc_insts.sh <output dir>}
mkdir -p $O
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $O/t.log 2>&1; tail -2 $O/t.log
timeout -k 10 200 python bench.py --full --no-cpu-baseline > $O/b_fastload.json 2>$O/b.err
python - "$O" <<'PY'
import json, sys
d=json.load(open(sys.argv[1] + "/b_fastload.json"))
print(d["value"], d["ms_per_step"], {k:v["avg_ms"] for k,v in d["roofline"]["per_kernel"].items()})
PY
export TMPDIR=/tmp
for P in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS" "SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM SQ_BUSY_CYCLES" "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAVE_CYCLES SQ_WAIT_INST_ANY" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_VMEM SQ_INST_CYCLES_VMEM"; do
  n=$(echo $P | tr ' ' '_' | cut -c1-40)
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $P -d $O/pmc_$n -o pmc --output-format csv -- python3 bench.py --no-cpu-baseline --steps 1 --warmup 1 --sample-every 0 > /dev/null 2>$O/pmc_$n.err || echo "pmc $n failed"
done
python tools/pmc_summary.py $O/pmc_* > $O/pmc_summary.txt
cat $O/pmc_summary.txt
