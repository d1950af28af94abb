#!/bin/bash
# usage: tools/round_measure.sh <tag> [part]   (on the GPU box, from the repo root): everything a round's RESULTS / profiles quote.
#   part 1: the GPU test suite, the default bench line with --full, the rocprofv3 passes of it (kernel stats, PMC traffic, SQ and LDS counters)
#   part 2: the configuration sweep, the streaming sweep, the clock probe
# (one part per GPU session when a session is limited to 20 minutes).  This script's logs go under out/<tag>/; the profile
# passes and the sweeps write where their own usage lines say (copy the summaries to profiles/).
TAG=$1
PART=${2:-all}
O=out/$TAG
mkdir -p $O
if [ "$PART" = 1 ] || [ "$PART" = all ]; then
  timeout -k 10 600 python -m pytest tests -x -q -m gpu > $O/gputests.log 2>&1; tail -2 $O/gputests.log
  timeout -k 10 300 python bench.py --full > $O/bench.json 2> $O/bench.err && echo "[round_measure] bench done"
  bash tools/profile_round.sh $TAG > $O/profile_round.log 2>&1; tail -3 $O/profile_round.log
fi
if [ "$PART" = 2 ] || [ "$PART" = all ]; then
  bash tools/sweep_configs.sh $TAG > $O/sweep_configs.log 2>&1; tail -20 $O/sweep_configs.log
  bash tools/sweep_streaming.sh $TAG > $O/sweep_streaming.log 2>&1; tail -9 $O/sweep_streaming.log
  bash tools/clock_probe.sh $O/clock > $O/clock_probe.txt 2>&1; cat $O/clock_probe.txt
fi
