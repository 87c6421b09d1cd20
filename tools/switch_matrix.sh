# usage (on an MI355X): bash tools/switch_matrix.sh  -> one line per fallback switch: 51 parity tests and the 13 VGG16 gradient
# gates of tests/test_gpu_vgg_grad.py under it; the logs go where the suite's GPU-run logs go (tools/run_gpu_children.py: OUT)
out=$(python -c "import sys; sys.path.insert(0, 'tools'); import run_gpu_children; print(run_gpu_children.OUT)") || exit 1
mkdir -p "$out"
for v in UMPR_MERGE_SMALL=0 UMPR_B16_POOL_BWD_WIN=0 UMPR_WINO_BIAS_FUSE=0 UMPR_FC_K32=0 UMPR_EMB_GATHER=0 UMPR_WINO_C21_FWD=0 UMPR_TEXT_STREAM=0 UMPR_WGRAD_STREAM=0 UMPR_WINO_FOLD=2 UMPR_WINO_V_REUSE=0 UMPR_POOL_FOLD=0; do
  env $v UMPR_TEST_CHILD=1 timeout -k 10 400 python -m pytest tests/test_gpu_parity.py tests/test_gpu_bf16.py tests/test_gpu_vgg_grad.py -q -m gpu -p no:cacheprovider -k "golden or review_head or control or embed_gru or umpr_r_small or trained or eval_mse or maxpool_bf16 or vgg16_small or classifier_at or vgg16_grad" > "$out/matrix_$v.log" 2>&1
  echo "$v: $(tail -1 "$out/matrix_$v.log")"
done
