#!/bin/bash
# The round's measurement set (~6 min of GPU time): GPU test suite, tools/profile_round.sh (bench line,
# rocprofv3 kernel stats, FETCH_SIZE / WRITE_SIZE / SQ_INSTS_VALU passes -> traffic.json, valu.json), every BASELINE config,
# the batch-size sweep, the drop-in single-stream bench, the host-memory bench, PV_ARITH_EXACT.  usage: tools/round_measure.sh
# <output dir>; outputs: <output dir>/z_* and tools/profile_round.sh's (tag r03/z); copy z_traffic.json / z_valu.json to
# profiles/ (their source hash must match the committed kernels) and the rest to profiles/r03/.
O=${1:?usage: tools/round_measure.sh <output dir>}
mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/z_gpu_tests.txt 2>&1; echo "suite rc $?"; tail -3 $O/z_gpu_tests.txt
bash tools/profile_round.sh r03/z
bash tools/bench_all.sh $O/z_bench_all_configs.txt > /dev/null; cat $O/z_bench_all_configs.txt | cut -c1-170
bash tools/streams_sweep.sh $O/z_streams_sweep.txt 4 8 20 32 64 97 128 160 192 > /dev/null; cut -c1-110 $O/z_streams_sweep.txt
./audiomod_amd/lib/stream_bench 60 480 2 > $O/z_dropin_stream_bench.json; ./audiomod_amd/lib/stream_bench 60 4800 2 >> $O/z_dropin_stream_bench.json; cat $O/z_dropin_stream_bench.json
timeout -k 10 300 python bench.py --host-io --no-cpu-baseline > $O/z_bench_hostio.json 2> $O/z_bench_hostio.err; python -c "
import json; l=json.loads(open('$O/z_bench_hostio.json').read().strip().splitlines()[-1]); print(l['host_io'])"
AUDIOMOD_PV_EXACT=1 timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/z_bench_exact.json 2> $O/z_bench_exact.err; python -c "
import json; l=json.loads(open('$O/z_bench_exact.json').read().strip().splitlines()[-1]); print('exact', l['value'], l['ms_per_step'], l['verified']['max_rms_vs_oracle'], l['verified']['batch_checksum_sha256'][:12])"
