#!/bin/bash
# Regenerates every measurement artefact under profiles/ from the tree it runs in (on a GPU box):
#   tools/regen_profiles.sh <round-tag, e.g. r04>      -> gpurun_out/<tag>/...   (copy into profiles/ afterwards)
# Passes: (1) SpMM PMC for the two headline shapes -> spmm_pmc_latest.json (AM, F = 10, k_spmm3) and
# spmm_pmc_fb15k.json (FB15k-237, F = 200, k_spmm<64>): the bench lines quote them (digest-checked),
# (2) the default bench line (headline + seeds 0-2 + the six side workloads under extra.workloads),
# (3) rocprofv3 --kernel-trace --stats of the same command -> kernel stats, trace medians, the epoch's launch sequence,
# (4) epoch PMC (memory + SQ sets) for the weight_I streamers and the transforms -> epoch_pmc.md and, with (3),
# kernel_roofline.md, (5) the fb15k line + its launch sequence, (6) the encoders' product probe + MFMA counters,
# (7) the next-rows probe (mini-batch incl. the masked pass, encoders, ingestion) + the launch sequence of one
# re-sampled mini-batch step, (8) the halo-size probe, (9) one replayed step of the full-multimodal model kernel by kernel.
tag=${1:-rXX}
cd ${GRAFT_REPO_ROOT:-.}
export TMPDIR=/tmp
o=gpurun_out/$tag
mkdir -p $o
bash tools/pmc_passes.sh $o/pmc_spmm mem -- python3 tools/spmm_probe.py --ld 10 --row-bytes 40 44 --iters 10
python3 tools/make_spmm_pmc_json.py $o/pmc_spmm "k_spmm3<" > $o/spmm_pmc_latest.json
python3 tools/pmc_summary.py $o k_spmm3 > $o/spmm_pmc.md
rm -rf $o/pmc_spmm_*/
bash tools/pmc_passes.sh $o/pmc_spfb mem -- python3 tools/spmm_probe.py --workload fb15k --F 200 --ld 200 --row-bytes 800 --iters 10
python3 tools/make_spmm_pmc_json.py $o/pmc_spfb "k_spmm<64" fb15k 200 > $o/spmm_pmc_fb15k.json
python3 tools/pmc_summary.py $o "k_spmm<64" > $o/spmm_pmc_fb15k.md
rm -rf $o/pmc_spfb_*/
cp $o/spmm_pmc_latest.json profiles/spmm_pmc_latest.json   # the bench lines quote them (digest-checked)
cp $o/spmm_pmc_fb15k.json profiles/spmm_pmc_fb15k.json
# clocks / power beside the bench line (one sample per 0.5 s while it runs; needs nothing but read access)
( for i in $(seq 1 400); do rocm-smi --showclocks --showpower --csv 2>/dev/null | tr '\n' ' '; echo; sleep 0.5; done > $o/rocm_smi_during_bench.txt ) &
smi_pid=$!
python3 bench.py --full > $o/bench_line.json 2> $o/bench_line.err
kill $smi_pid 2>/dev/null; wait $smi_pid 2>/dev/null
rocprofv3 --kernel-trace --stats --output-format csv -d $o/stats -o run -- python3 bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-renumbered-extra --no-reference-loop --no-seeds --no-side-workloads > $o/bench_under_rocprof.json 2> $o/bench_under_rocprof.err
python3 tools/prof_summary.py $o/stats 40 > $o/epoch_kernel_stats.md
python3 tools/trace_summary.py $o/stats > $o/epoch_kernel_trace_medians.md 2>/dev/null
python3 tools/epoch_sequence.py $o/stats "k_xform_mfma_fwd<1, false, 10" > $o/epoch_sequence.md 2>/dev/null
bash tools/pmc_passes.sh $o/pmc_epoch all -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-renumbered-extra --no-reference-loop --no-literal-spmm --no-graph --no-seeds --no-side-workloads
for k in k_mix_fwd k_mix_bwd_sup k_dcomp k_adam_rows k_xform_mfma_fwd k_xform_cols_lds k_xform_mfma_dw "k_spmm<" k_spmm3; do
  echo "## $k"; python3 tools/pmc_summary.py $o "$k" | tail -n +3
done > $o/epoch_pmc.md
python3 tools/roofline_table.py $o/stats $o/bench_line.json $o > $o/kernel_roofline.md 2> $o/kernel_roofline.err
rm -rf $o/stats $o/pmc_epoch_*/
python3 bench.py --full --workload fb15k > $o/bench_fb15k.json 2> $o/bench_fb15k.err
rocprofv3 --kernel-trace --stats --output-format csv -d $o/stats_lp -o run -- python3 bench.py --full --workload fb15k --steps 20 --warmup 3 --no-cpu-baseline > /dev/null 2> $o/bench_fb15k_prof.err
python3 tools/epoch_sequence.py $o/stats_lp k_corrupt_triples > $o/lp_epoch_sequence.md 2>&1
rm -rf $o/stats_lp
# (6) the encoders' tiled product over the TCNN-M shapes: per-product rates, MFMA counters; (7) the next-rows probe
python3 tools/gemm_probe.py > $o/gemm_probe.txt 2> $o/gemm_probe.err
python3 tools/gemm_probe.py --mm bf16 >> $o/gemm_probe.txt 2>> $o/gemm_probe.err
python3 tools/gemm_probe.py --json > $o/gemm_probe.json 2>> $o/gemm_probe.err
bash tools/pmc_passes.sh $o/pmc_mm mfma -- python3 tools/gemm_probe.py --iters 3
python3 tools/pmc_summary.py $o k_mm_tile > $o/mfma_mm.md
rm -rf $o/pmc_mm_*/
python3 tools/next_rows_probe.py > $o/next_rows.json 2> $o/next_rows.err
rocprofv3 --kernel-trace --stats --output-format csv -d $o/stats_mb -o run -- python3 tools/minibatch_step.py 10 > $o/minibatch_step.txt 2> $o/minibatch_step.err
python3 tools/epoch_sequence.py $o/stats_mb k_sup_rowcount 2 > $o/minibatch_step_sequence.md 2>&1
rm -rf $o/stats_mb
python3 tools/halo_probe.py > $o/halo.json 2> $o/halo.err
rocprofv3 --kernel-trace --output-format csv -d $o/stats_enc -o run -- python3 tools/am_encoders_step.py run > $o/am_encoders_step.txt 2> $o/am_encoders_step.err
python3 tools/am_encoders_step.py summary $o/stats_enc > $o/am_encoders_step.md 2>> $o/am_encoders_step.err
rm -rf $o/stats_enc
rocprofv3 --kernel-trace --output-format csv -d $o/stats_encb -o run -- python3 tools/am_encoders_step.py run bf16 > $o/am_encoders_step_bf16.txt 2> $o/am_encoders_step_bf16.err
python3 tools/am_encoders_step.py summary $o/stats_encb > $o/am_encoders_step_bf16.md 2>> $o/am_encoders_step_bf16.err
rm -rf $o/stats_encb
# (10) the bf16 pipeline's epoch in launch order; (11) the yardstick and LDS labs (tools/lab)
rocprofv3 --kernel-trace --stats --output-format csv -d $o/stats_bf16 -o run -- python3 bench.py --full --operand bf16 --steps 20 --warmup 3 --no-cpu-baseline --no-renumbered-extra --no-reference-loop --no-seeds --no-side-workloads --no-literal-spmm > $o/bench_bf16_under_rocprof.json 2> $o/bench_bf16_under_rocprof.err
python3 tools/epoch_sequence.py $o/stats_bf16 k_xform_bf16_fwd > $o/bf16_epoch_sequence.md 2>&1
rm -rf $o/stats_bf16
# (10b) the small graphs' replayed epochs in launch order (BASELINE configs 1 and 2: launch-bound)
for w in aifb mutag; do
  rocprofv3 --kernel-trace --stats --output-format csv -d $o/stats_$w -o run -- python3 bench.py --full --workload $w --steps 50 --warmup 5 --no-cpu-baseline --no-renumbered-extra --no-reference-loop --no-seeds --no-side-workloads --no-literal-spmm > $o/bench_${w}_under_rocprof.json 2> $o/bench_${w}_under_rocprof.err
  python3 tools/epoch_sequence.py $o/stats_$w k_xent_rows shortest > $o/${w}_epoch_sequence.md 2>&1
  rm -rf $o/stats_$w
done
# (10c) node dropout: the replayed epoch with p = 0 and with the device draw, the eager epoch with the host draw.
# Row (a) of DESIGN section 12 is the PARENT commit's p = 0 epoch on the same box: check the parent out beside this tree,
# build it, copy tools/node_dropout_probe.py into it and run `python3 tools/node_dropout_probe.py --rows p0 --out <file>`
# there first; NODE_DROPOUT_PARENT_JSON=<file> then puts that row into the result.  Without it the file holds no row (a).
python3 tools/node_dropout_probe.py ${NODE_DROPOUT_PARENT_JSON:+--parent $NODE_DROPOUT_PARENT_JSON} --out $o/node_dropout_probe.json > $o/node_dropout_probe.txt 2> $o/node_dropout_probe.err
# (10d) top-k completion at the FB15k-237 decoder shape: predict_topk, torch.topk over the score matrix, compute_ranks_fast
python3 tools/lp_topk_probe.py --out $o/lp_topk_probe.json > $o/lp_topk_probe.txt 2> $o/lp_topk_probe.err
# (10e) validation and early stopping inside the replayed epoch against the host loop around a replayed train step
python3 tools/early_stop_probe.py --out $o/early_stop_probe.json > $o/early_stop_probe.txt 2> $o/early_stop_probe.err
# (10f) weight decay / L1 / L2 on the row-sparse node-table step.  The baseline rows are the PARENT commit's on the same box:
# check the parent out beside this tree, build it, copy tools/weight_reg_probe.py into it and run
# `python3 tools/weight_reg_probe.py --rows-only --zero-repeats 3 --out <file>` there first; WEIGHT_REG_PARENT_JSON=<file>
# then puts them into the result.  Without it the file holds this tree's rows only.
python3 tools/weight_reg_probe.py ${WEIGHT_REG_PARENT_JSON:+--parent $WEIGHT_REG_PARENT_JSON} --out $o/weight_reg_probe.json > $o/weight_reg_probe.txt 2> $o/weight_reg_probe.err
# (10g) link prediction's run loop on the device: rank_both against the two rank calls, the replayed evaluating epoch
# against the host loop, the replayed training epoch against GraphedStep
python3 tools/lp_fit_probe.py --out $o/lp_fit_probe.json > $o/lp_fit_probe.txt 2> $o/lp_fit_probe.err
# (10h) the mini-batch node-classification run loop at the AM/4 shape, batches of 1 024 and of 64: the replayed epoch, the
# eager device epoch, the loop as the reference writes it, the fused loss launch against the two it replaces
python3 tools/nc_minibatch_probe.py --out $o/nc_minibatch_probe.json > $o/nc_minibatch_probe.txt 2> $o/nc_minibatch_probe.err
# (10i) the mini-batch link-prediction run loop at the FB15k-237 shape: batch_eval against the two sequences it replaces,
# eval_batches against evaluate_batches, the eager device epochs against the host loop
python3 tools/lp_minibatch_fit_probe.py --out $o/lp_minibatch_fit_probe.json > $o/lp_minibatch_fit_probe.txt 2> $o/lp_minibatch_fit_probe.err
# (10j) the L1 / L2 weight penalty of the link-prediction loops at the FB15k-237 shape: the step, a whole training epoch
# and a replayed full-batch epoch without penalties, with the penalty inside the optimizer's step, and with it written
# into the loss by hand
python3 tools/lp_penalty_probe.py --out $o/lp_penalty_probe.json > $o/lp_penalty_probe.txt 2> $o/lp_penalty_probe.err
# (10k) keyed, filtered negatives at the FB15k-237 shape: the sampler call at 1 and 10 negatives per fact, filtered and
# unfiltered, next to the default sampler's; the replayed training epoch of fit with each.  The parent rows of DESIGN
# section 19 are the PARENT commit's on the same box: check the parent out beside this tree, build it, copy
# tools/lp_negatives_probe.py into it and run `python3 tools/lp_negatives_probe.py --rows default --out <file>` there
# first; LP_NEGATIVES_PARENT_JSON=<file> then puts them into the result.  Without it the file holds this tree's rows only.
python3 tools/lp_negatives_probe.py ${LP_NEGATIVES_PARENT_JSON:+--parent $LP_NEGATIVES_PARENT_JSON} --out $o/lp_negatives_probe.json > $o/lp_negatives_probe.txt 2> $o/lp_negatives_probe.err
# (10l) the grouped decoder next to the flat one at the FB15k-237 shape, 1 and 10 keyed negatives per fact: the replayed
# training epoch of fit (also with a positive weight and with the softmax loss), scores + loss alone, the backward alone,
# the median mini-batch's step.  The parent rows of DESIGN section 20 are the PARENT commit's on the same box: check the
# parent out beside this tree, build it, copy tools/lp_grouped_probe.py into it and run
# `python3 tools/lp_grouped_probe.py --rows triples --out <file>` there first; LP_GROUPED_PARENT_JSON=<file> then puts
# them into the result.  Without it the file holds this tree's rows only.
python3 tools/lp_grouped_probe.py ${LP_GROUPED_PARENT_JSON:+--parent $LP_GROUPED_PARENT_JSON} --out $o/lp_grouped_probe.json > $o/lp_grouped_probe.txt 2> $o/lp_grouped_probe.err
# (10m) the ComplEx scorer next to DistMult at the FB15k-237 shape: flat scores + BCE, the backward alone (DistMult's
# default and deterministic routes, ComplEx's one fixed-order route), rank_both over the validation-sized fact set,
# predict_topk of 500 queries at k = 10, the replayed training epoch of fit; DistMult's rows again at the end
python3 tools/lp_complex_probe.py --out $o/lp_complex_probe.json > $o/lp_complex_probe.txt 2> $o/lp_complex_probe.err
# (10n) the 1-vs-all softmax decoder at the FB15k-237 shape: all_loss forward / backward and its three kernels alone
# (with their TFLOP/s) at 4 096, 32 768 and all 272 115 facts next to F.cross_entropy on the materialised matrix where
# that fits, the replayed training epoch of fit with decoder="all" against decoder="grouped" at 10 negatives, the median
# mini-batch's step; every leg in a child process under its own time limit
python3 tools/lp_all_probe.py --out $o/lp_all_probe.json > $o/lp_all_probe.txt 2> $o/lp_all_probe.err
# (10n') the KvsAll decoder at the FB15k-237 shape beside the 1-vs-all one in the same run (`all_loss` first and last):
# kvsall_loss forward and backward with the queries' m, nnz and m / 2n, the kernels alone with their per-query ratio to
# lp_all's, torch's materialised BCE where it fits with both peak memories, the replayed fit epoch with
# decoder="kvsall" (label_smoothing 0 and 0.1) beside the untouched decoders, the median mini-batch's step.  The
# untouched decoders' band is the PARENT commit's on the same box: check the parent out beside this tree, build it, copy
# tools/lp_kvsall_probe.py into it and run `python3 tools/lp_kvsall_probe.py --legs epoch_untouched
# batch_step_untouched --out <this tree>/profiles/lp_kvsall_probe_parent.json` there.
python3 tools/lp_kvsall_probe.py --out $o/lp_kvsall_probe.json > $o/lp_kvsall_probe.txt 2> $o/lp_kvsall_probe.err
# (10n'') the bf16 score arithmetic of both all-candidates decoders beside the f32 arithmetic in the same run: the C
# entries alone (forward, dQ, dE, forward + backward, TFLOP/s) at all 272 115, 32 768 and 4 096 facts and at the median
# mini-batch's shape, the bf16 tables' bytes and casts, torch's materialised route in fp32 and under bf16 autocast, the
# replayed fit epoch of both decoders under both settings.  The f32 rows' band is the PARENT commit's on the same box:
# check the parent out beside this tree, build it, copy tools/lp_bf16_probe.py into it and run `python3
# tools/lp_bf16_probe.py --f32-only --out <this tree>/profiles/lp_bf16_probe_parent.json` there.  The resource table:
# `python3 tools/kernel_resources.py mrgcn_amd/csrc/lp_all.hip bf16` and the same for lp_kvsall.hip ->
# profiles/lp_bf16_kernels.md
python3 tools/lp_bf16_probe.py --out $o/lp_bf16_probe.json > $o/lp_bf16_probe.txt 2> $o/lp_bf16_probe.err
# (10o) a block-diagonal hidden layer (200 -> 200, 40 blocks) at the FB15k-237 shape: its five passes alone, the layer on
# the fused engine against the literal engine on the dense expansion (with peak memory), the replayed two-layer fit epoch
python3 tools/block_layer_probe.py --out $o/block_layer_probe.json > $o/block_layer_probe.txt 2> $o/block_layer_probe.err
# (10p) edge dropout: one layer's draw alone and the replayed fit epoch with it on and off, FB15k-237 and AM shapes
# (run the same script in a checkout of the parent commit for profiles/edge_dropout_probe_parent.json)
python3 tools/edge_dropout_probe.py --out $o/edge_dropout_probe.json > $o/edge_dropout_probe.txt 2> $o/edge_dropout_probe.err
hipcc -O3 --offload-arch=gfx950 -std=c++17 tools/lab/copy_lab.hip -o /tmp/copy_lab 2>/dev/null && /tmp/copy_lab > $o/copy_lab.txt 2>&1
python3 tools/lab/spmm_hot_lab.py > $o/spmm_hot_lab.txt 2>&1
# the CPU suite last: the tree these artefacts describe is green
python3 -m pytest tests -q -x -m "not gpu" > $o/cpu_suite.txt 2>&1; tail -2 $o/cpu_suite.txt
ls -la $o
# (12) the driver's multi-rank command with two ranks on this one GPU (gloo: the ranks share the device, so the times
# are time-shared upper bounds): both partitioned engines priced, logits against the single-GPU model
timeout 900 python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 5 --warmup 2 --no-cpu-baseline --no-renumbered-extra --no-reference-loop --no-seeds --no-side-workloads --no-literal-spmm > $o/bench_two_ranks_one_gpu.json 2> $o/bench_two_ranks_one_gpu.err
ls -la $o
