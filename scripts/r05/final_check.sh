# the round's evidence at the current code: full GPU suite, smoke(), the driver's bench line, profile set
cd $GRAFT_REPO_ROOT && export TMPDIR=/tmp && mkdir -p gpurun_out &&
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/smoke.log 2>&1 && cat gpurun_out/smoke.log &&
bash scripts/gpu_run.sh tests "bench=--full --steps 20 --warmup 5" &&
bash scripts/round_profiles.sh 1 && cp gpurun_out/pmc_round.json profiles/pmc_latest.json && bash scripts/round_profiles.sh 2
