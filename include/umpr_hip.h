/* libumpr_hip.so - C ABI of the MI355X-native UMPR hot path.
 *
 * The reference (iamwinter/UMPR) has no FFI layer: its hot path is the Python nn.Module API of src/model.py
 * (UMPR.__init__ model.py:233-255, UMPR.forward model.py:257-278) and all arithmetic runs inside torch ATen /
 * torchvision.  This header is the boundary a maintainer binds instead (ctypes stub in INTEGRATION.md): each
 * entry point replaces the torch ops of the cited reference lines with hand-written gfx950 kernels.
 *
 * Conventions: every pointer is DEVICE memory owned by the caller (plain pointers and sizes, no torch types);
 * fp32 unless noted; token ids are int64 (the reference's LongTensor); lengths / permutations are int32 arrays the
 * host computes (the reference keeps lengths on the host too, model.py:18); `stream` is a hipStream_t passed as
 * void*; workspaces come from the caller (size queries below) - the library never allocates or frees.
 * Return value: 0 = ok, <0 = error (message: umpr_last_error(), thread-local).  Hidden sizes are the reference's
 * configuration constants: gru_size 64 (2u = 128), self_atte_size 64 (config.py:34-35).
 */
#ifndef UMPR_HIP_H
#define UMPR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* umpr_version(void);
const char* umpr_last_error(void);
/* name of device `dev`, number of CUs, bytes of HBM; used by bench.py to print what it ran on */
int umpr_device_info(int dev, char* name, int name_len, int* compute_units, size_t* hbm_bytes);

/* ---- generic fp32 MFMA GEMM: C = act(alpha * op(A) op(B) + bias + (accumulate ? C : 0)) --------------------
 * Replaces torch.mm/addmm/Linear call sites on the path (model.py:50,75,120,154-155,167-168; VGG classifier).
 * op(A)(m,k) = transA ? A[k*lda+m] : A[m*lda+k];  op(B)(k,n) = transB ? B[n*ldb+k] : B[k*ldb+n].
 * bias_mode: 0 none, 1 bias[n], 2 bias[m].  act: 0 none, 1 relu, 2 tanh, 3 sigmoid.
 * ws/ws_bytes: optional split-K workspace (used when the grid would not fill the GPU).  A workspace too small for the chosen
 * split is used for as many slabs of M * N floats as fit, one slab or less means no split; nothing is written behind ws_bytes.
 * K = 0 is accepted and gives C = act(bias + (accumulate ? C : 0)).  lda / ldb / ldc may exceed the row length and the bases
 * need no alignment (16-byte loads are used only where base, pitch and extent allow them); the gap columns of a C with
 * ldc > N are never written.  Every element of C[0..M)[0..N) is written by the call. */
int umpr_gemm_f32(const float* A, long lda, int transA, const float* B, long ldb, int transB, float* C, long ldc,
                  int M, int N, int K, const float* bias, int bias_mode, int act, int accumulate, float alpha,
                  float* ws, size_t ws_bytes, void* stream);

/* Mixed precision for the GEMM-shaped products of the text path (BASELINE.json configs[4]; not in the reference, which
 * would get it from torch.autocast): while set on the calling host thread, every product the library issues through this
 * GEMM (GRU input projections, co-attention / S-Net / C-Net projections and their gradients) rounds its operands to bf16 on
 * the way into LDS and runs on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Set it around a call, clear it after. */
int umpr_set_gemm_bf16(int on);

/* Inference hint for the fp32 convolution stack (the reference's counterpart is torch.no_grad() around evaluate.py:8-13):
 * while set on the calling host thread, forward convolutions may use the F(4x4,3x3) Winograd tile that training reserves for
 * the backward pass - its rounding (5e-6 of max|y|) is irrelevant when no gradient will be taken through the ReLU / pool
 * decisions of this forward.  Predictions move by ~3e-6.  Set it around umpr_vgg16_features_fwd / umpr_conv3x3_fwd. */
int umpr_set_conv_inference(int on);

/* A 2x2 max-pool will consume the output of the next umpr_conv3x3_fwd calls of this host thread (umpr_vgg16_features_fwd sets
 * it itself around conv3_3 / conv4_3 / conv5_3): the decision fix-up of the F(4x4,3x3) training forward (winograd.hip) then
 * covers the pool windows' argmax as well as the ReLU signs.  Callers that chain umpr_conv3x3_fwd + umpr_maxpool2_fwd
 * themselves set it likewise. */
int umpr_set_conv_pool_follows(int on);

/* Test / tooling aid: number of outputs the most recent decision fix-up pass of this host thread listed for recomputation
 * (-1: none yet).  Synchronises the device. */
long umpr_debug_wino_fix_count(void);

/* Test / tooling aid: what the fp32 3x3 convolution dispatch decides for one pass (0 forward, 1 data gradient, 2 weight gradient)
 * of one layer shape, `inference` as under umpr_set_conv_inference.  Returns the algorithm: 0 generic gather kernels, 1
 * first-layer kernels, 2 LDS-patch direct kernels, 3 Winograd F(2x2,3x3), 4 Winograd F(4x4,3x3); <0 on bad arguments.
 * *ws_bytes: scratch the pass reserves (never more than umpr_conv3x3_pack_bytes / umpr_conv3x3_bwd_weight_ws_bytes return);
 * *v_bytes: size of the transformed input the training forward keeps in the activation arena for the weight gradient (0: none).
 * Pure host arithmetic: makes no HIP call, runs without a GPU. */
int umpr_debug_conv3x3_plan(int pass, int N, int Cin, int Cout, int H, int W, int inference, size_t* ws_bytes, size_t* v_bytes);
/* The same for the bf16 per-layer entry points (umpr_conv3x3_bf16_fwd / _bwd_data / _bwd_weight below): the launch of one pass,
 * from the very functions the launchers build it with.  Returns 0 and fills out[0..9]; < 0 where the entry point would refuse the
 * shape (umpr_last_error names the cause).  Pure host arithmetic, no HIP call.
 *   pass 0 / 1: out[0] BN (output channels per workgroup: 64, 128 or 256), [1] nct output-channel tiles, [2] ntp pixel tiles,
 *     [3] workgroups launched, [4] grid rule (0: nct divides 8 and an XCD keeps one channel tile; 1: channel tiles interleaved
 *     along an XCD's slots), [5] 32-channel chunks of the reduction, [6] 1 on the 2-D pixel tile (224 / 112 maps), [7] 1 under
 *     the ping-pong schedule, [8] bytes of scratch the pass needs, [9] 0.
 *   pass 2: out[0] 1 on the 128 x 64 channel tile (0: 64 x 64, two k-groups), [1] nseg pixel segments, [2] ntiles channel tiles,
 *     [3] splits, [4] segments per split, [5] segments of the last split, [6] workgroups launched (those behind `splits`
 *     idle), [7] 1 on the wide reduce (splits >= 32; 0: linear), [8] bytes of scratch, [9] ncit input-channel tiles. */
int umpr_debug_conv_bf16_plan(int pass, int N, int Cin, int Cout, int H, int W, long* out);

/* Test aid: the gradients of one conv layer that a 2x2 max-pool follows, on the Winograd kernels whatever the plan says for the
 * shape (H, W even; f4 = 1: the 4x4 tile, H and W multiples of 4 or, data gradient only, any even size; f4 = 0: the 2x2 tile,
 * weight gradient only).  y [N][Cout][H][W] is the layer's output, g_pooled [N][Cout][H/2][W/2] the gradient of the pooled map.
 * fold = 1: the gradient readers form the un-pooled gradient themselves (what umpr_vgg16_features_bwd does for pools 2-5);
 * fold = 0: umpr_maxpool2_bwd_relu writes it to `unpooled` [N][Cout][H][W] first and the same kernels read that.
 * dx [N][Cin][H][W] (NULL: no data gradient, else f4 must be 1), dw [Cout][Cin][3][3] + db [Cout] (dw NULL: no weight gradient;
 * x [N][Cin][H][W] is the layer's input).  ws: scratch of ws_bytes; the call fails if it is too small. */
int umpr_debug_wino_pool_fold(const float* y, const float* g_pooled, const float* w, const float* x, float* unpooled, float* dx,
                              float* dw, float* db, int N, int Cin, int Cout, int H, int W, int f4, int fold, float* ws,
                              size_t ws_bytes, void* stream);

/* ---- K1-K3: embedding lookup + bidirectional packed GRU + the reference's double un-sort ---------------------
 * Replaces nn.Embedding (model.py:262-264) + ImprovedRnn.forward (model.py:12-21) for one review tensor.
 * ids [N*L] int64; emb [vocab][E]; GRU weights in nn.GRU layout (gate order r,z,n): w_ih [192][E], w_hh [192][64],
 * b_ih/b_hh [192], forward direction then "_reverse".  lengths [N]; order [N] = sorted_indices (descending length,
 * the tie order torch.sort produced); dst_row [N]: input row n lands in output row dst_row[n] (= sorted_indices[n]
 * for the reference's semantics; must be a permutation of 0..N-1: each output row is written - values up to its length, zeros
 * past it - by the sequence that owns it).  out [N][L][128] (zeros past each length).  saved [2][N][L][4][64] (gates for
 * backward) or NULL for inference.
 * Pinned by tests/test_gpu_gru.py against a float64 recurrence: a length of 0 yields an all-zero output row and no gradient; a
 * length above L is treated as L; `order` and `dst_row` are independent (a sequence's values do not depend on either);
 * saved[dir][n][t] = (r, z, n, W_hn h + b_hn) is indexed by INPUT row n and is defined only for t < length - the forward leaves
 * the rest untouched, and no value of saved or dout at t >= length reaches the backward's results.  Every byte of out, of the
 * gradients and of the workspace that a call uses was written by that call: none of them needs to be cleared. */
size_t umpr_embed_gru_bidir_ws_bytes(int N, int L, int E);
int umpr_embed_gru_bidir_fwd(const int64_t* ids, const float* emb, int E,
                             const float* w_ih_f, const float* w_hh_f, const float* b_ih_f, const float* b_hh_f,
                             const float* w_ih_r, const float* w_hh_r, const float* b_ih_r, const float* b_hh_r,
                             const int32_t* lengths, const int32_t* order, const int32_t* dst_row, int N, int L,
                             float* out, float* saved, float* ws, size_t ws_bytes, void* stream);
/* dout [N][L][128]; d* receive the parameter gradients (overwritten).  No gradient is produced for the embedding table (the
 * reference's default: nn.Embedding.from_pretrained, model.py:237); umpr_embed_gru_bidir_bwd_dx below hands out the token
 * gradient a trainable table needs. */
int umpr_embed_gru_bidir_bwd(const int64_t* ids, const float* emb, int E,
                             const float* w_hh_f, const float* w_hh_r,
                             const int32_t* lengths, const int32_t* order, const int32_t* dst_row, int N, int L,
                             const float* dout, const float* out, const float* saved,
                             float* dw_ih_f, float* dw_hh_f, float* db_ih_f, float* db_hh_f,
                             float* dw_ih_r, float* dw_hh_r, float* db_ih_r, float* db_hh_r,
                             float* ws, size_t ws_bytes, void* stream);

/* The same with `accumulate` != 0 adding onto the eight gradient buffers instead of overwriting them: the reference uses
 * ONE GRU for user and item reviews (model.py:45-46) and one for the three C-Net calls (model.py:182-184); a caller that
 * owns flat gradient storage lets the second and third call accumulate in place instead of adding temporaries. */
int umpr_embed_gru_bidir_bwd_acc(const int64_t* ids, const float* emb, int E,
                                 const float* w_hh_f, const float* w_hh_r,
                                 const int32_t* lengths, const int32_t* order, const int32_t* dst_row, int N, int L,
                                 const float* dout, const float* out, const float* saved,
                                 float* dw_ih_f, float* dw_hh_f, float* db_ih_f, float* db_hh_f,
                                 float* dw_ih_r, float* dw_hh_r, float* db_ih_r, float* db_hh_r,
                                 int accumulate, float* ws, size_t ws_bytes, void* stream);

/* The same, and the gradient of the embedded tokens for a TRAINABLE table (nn.Embedding.from_pretrained(..., freeze=False)):
 * dx [N*L][E] = dgx[:, 0:192] W_ih_f + dgx[:, 192:384] W_ih_r, overwritten (dx_accumulate = 0) or added onto (!= 0).  Two products
 * on the generic GEMM, in fp32 whatever umpr_set_gemm_bf16 says.  Positions past a sequence's length receive exact zeros (their
 * dgx is zero).  dx = NULL: w_ih_* are not read and the call is umpr_embed_gru_bidir_bwd_acc launch for launch; the eight
 * parameter gradients are bit-identical either way.  Same workspace (umpr_embed_gru_bidir_ws_bytes). */
int umpr_embed_gru_bidir_bwd_dx(const int64_t* ids, const float* emb, int E,
                                const float* w_hh_f, const float* w_hh_r,
                                const int32_t* lengths, const int32_t* order, const int32_t* dst_row, int N, int L,
                                const float* dout, const float* out, const float* saved,
                                float* dw_ih_f, float* dw_hh_f, float* db_ih_f, float* db_hh_f,
                                float* dw_ih_r, float* dw_hh_r, float* db_ih_r, float* db_hh_r,
                                int accumulate, const float* w_ih_f, const float* w_ih_r, float* dx, int dx_accumulate,
                                float* ws, size_t ws_bytes, void* stream);

/* ---- gradient of the embedding table: d_emb [vocab][E] = scatter-add of token gradients, deterministic, no atomics ----------
 * Up to 4 sources k of T_k tokens each: ids[k] int64 [T_k], dx[k] fp32 [T_k][E] (what umpr_embed_gru_bidir_bwd_dx and the two
 * *_net_bwd_dx calls hand out).  ids / dx / counts are HOST arrays of n_src device pointers / token counts, read during the
 * call.  sorted_pos: device int32 [T], T = sum of T_k - the positions 0..T-1 of the concatenated sources, STABLE-sorted by id
 * (torch.sort(cat(ids), stable=True).indices as int32).
 * d_emb is OVERWRITTEN WHOLE: every row is written exactly once, a row no token names becomes +0.0 (no zeroing pass is needed
 * before the call).  Row v = the sum of dx over the positions whose id is v, chained in fp32 from +0.0 in ascending position
 * order; the sorted order is cut at every multiple of umpr_embed_grad_chunk() positions, a run of one id that crosses such a cut
 * is summed piece by piece and the pieces are then added in order.  Where the cuts fall is a function of the sorted ids alone -
 * not of the grid, the scheduling or the device - so the result is bit-reproducible (the rule of umpr_grad_norm), and the same
 * tokens give the same bits however they are split into sources.
 * Ids live in device memory, so none is known to the host and none is refused: an id outside [0, vocab) contributes to NO row
 * and nothing is written for it.  A sorted_pos entry outside [0, T) is skipped likewise; with a sorted_pos that is not the
 * stable sort the values are unspecified, but no access leaves the buffers.  T = 0 (or n_src = 0) gives an all-zero table and
 * needs no workspace.  Any E >= 1 and vocab >= 1; row offsets are 64-bit; T < 2^31 - 512.
 * ws: umpr_embed_grad_ws_bytes(T, E) bytes, 8-byte aligned (pure host arithmetic: the ids behind the sorted positions, two
 * piece sums per umpr_embed_grad_chunk() positions).  No allocation, no copy, no host synchronisation: capture-safe. */
int umpr_embed_grad_chunk(void);
size_t umpr_embed_grad_ws_bytes(long T, int E);
int umpr_embed_grad(const int64_t* const* ids, const float* const* dx, const long* counts, int n_src, int E, long vocab,
                    const int32_t* sorted_pos, float* d_emb, void* ws, size_t ws_bytes, void* stream);

/* ---- the same gradient kept SPARSE, and row-wise Adam on the rows it names (torch.optim.SparseAdam on nn.Embedding(sparse=True))
 * umpr_embed_grad_rows: sources, sorted_pos, E and vocab as for umpr_embed_grad.  Outputs over the T SORTED positions: row_id
 * int64 [T], row_grad fp32 [T][E].  Every position j is written exactly once: if j begins a run (of equal ids) whose id lies in
 * [0, vocab), row_id[j] is that id and row_grad[j] the run's sum - BIT-EQUAL to the row umpr_embed_grad writes for the same
 * inputs (the same cuts, the same order inside a piece and over the pieces); otherwise row_id[j] = -1 and row_grad[j] is +0.0 in
 * every column, so the whole of row_grad can be one more arena of umpr_grad_norm.  Nothing of size vocab is read or written; no
 * atomics.  T = 0 is a successful no-op (row_id / row_grad / ws may be NULL).  Refused before any launch: a null source table or
 * source, a null sorted_pos / row_id / row_grad with T > 0, E < 1, vocab < 1, a workspace below
 * umpr_embed_grad_rows_ws_bytes(T, E) bytes or not 8-byte aligned.  No allocation, no copy, no host synchronisation.
 *
 * umpr_sparse_adam_rows: for every j in [0, T) with 0 <= row_id[j] < vocab, and g = row_grad[j] * grad_scale,
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;  p -= lr sqrt(1 - beta2^step) / (1 - beta1^step) * m / (sqrt(v) + eps)
 * on row row_id[j] of p, m, v [vocab][E] - SparseAdam's form: eps is added to sqrt(v) itself, there is no weight decay, and a row
 * no j names keeps every byte of p, m and v.  The row ids must be distinct (umpr_embed_grad_rows makes them so): each row is then
 * read and written by one wave alone.  clip_state: NULL, or the 8-float state of umpr_grad_norm - the scale is then the one float
 * product grad_scale * state[COEF] (COEF == 1: bit-identical to NULL) and state[FINITE] == 0 writes nothing.  p, m, v: any
 * float-aligned base.  Refused before the launch: E < 1, vocab < 1, step < 1, T < 0, a null pointer with T > 0; T = 0 is a
 * successful no-op.  No allocation, no copy: capture-safe. */
size_t umpr_embed_grad_rows_ws_bytes(long T, int E);
int umpr_embed_grad_rows(const int64_t* const* ids, const float* const* dx, const long* counts, int n_src, int E, long vocab,
                         const int32_t* sorted_pos, int64_t* row_id, float* row_grad, void* ws, size_t ws_bytes, void* stream);
int umpr_sparse_adam_rows(float* p, float* m, float* v, long vocab, int E, const int64_t* row_id, const float* row_grad, long T,
                          double lr, double beta1, double beta2, double eps, long step, double grad_scale,
                          const float* clip_state /*or NULL*/, void* stream);

/* ---- K4-K5: R-Net co-attention (model.py:50-55) --------------------------------------------------------------
 * Gu, Gi [B][SL][128]; M [128][128].  Outputs soft_u/soft_i [B][SL], atte_u/atte_i rows of 128 written at
 * atte_x + b*ld_x (lets the caller place them inside the [B][256] concat of model.py:166-167).
 * Saved for backward: T [B][SL][128], colmax/rowmax [B][SL], argcol/argrow [B][SL] int32. */
size_t umpr_coattention_fwd_ws_bytes(int B, int SL);
int umpr_coattention_fwd(const float* Gu, const float* Gi, const float* M, int B, int SL, float* T, float* soft_u,
                         float* soft_i, float* atte_u, long ld_u, float* atte_i, long ld_i, float* colmax,
                         int32_t* argcol, float* rowmax, int32_t* argrow, float* ws, size_t ws_bytes, void* stream);
/* The same with the score contraction tanh(T G_u^T) on bf16 MFMA (operands rounded to bf16, fp32 accumulation; tanh,
 * max, argmax, softmax in fp32) - the "attention" half of BASELINE.json configs[4].  Same outputs / saved tensors, and
 * umpr_coattention_bwd consumes them unchanged. */
int umpr_coattention_fwd_bf16(const float* Gu, const float* Gi, const float* M, int B, int SL, float* T, float* soft_u,
                              float* soft_i, float* atte_u, long ld_u, float* atte_i, long ld_i, float* colmax,
                              int32_t* argcol, float* rowmax, int32_t* argrow, float* ws, size_t ws_bytes, void* stream);
/* Token validity for the masked forms below: valid[n][l] = l < min(max(lengths[n], 0), L) && ids[n][l] != pad_id, one uint8
 * per token of ids [N][L].  One launch, no allocation, copy or host synchronisation (safe inside a stream capture).  Null
 * pointers and N or L below 1 are refused before the launch. */
int umpr_token_mask(const int64_t* ids, const int32_t* lengths, int N, int L, long pad_id, uint8_t* valid, void* stream);
/* umpr_coattention_fwd (bf16_scores = 0) or _fwd_bf16 (1) with a key-padding mask: valid_u / valid_i [B][SL] bytes for the user
 * (column) and item (row) positions.  colmax[k] / argcol[k] run over the valid item positions only (first one on ties) and are
 * defined when k is valid and some item position is; otherwise colmax[k] = +0.0, argcol[k] = -1.  soft_u is the softmax of
 * colmax over the defined positions and +0.0 elsewhere; a sample without any gets soft_u = 0 and atte_u = 0, never NaN.  Rows,
 * soft_i, atte_i alike.  With every byte set each output has the bits of the unmasked call.  Same three launches, same workspace
 * size; umpr_coattention_bwd consumes the saved tensors unchanged (gradients of masked rows come out as +0.0). */
int umpr_coattention_fwd_masked(const float* Gu, const float* Gi, const float* M, int B, int SL, float* T, float* soft_u,
                                float* soft_i, float* atte_u, long ld_u, float* atte_i, long ld_i, float* colmax,
                                int32_t* argcol, float* rowmax, int32_t* argrow, const uint8_t* valid_u,
                                const uint8_t* valid_i, int bf16_scores, float* ws, size_t ws_bytes, void* stream);
size_t umpr_coattention_bwd_ws_bytes(int B, int SL);
int umpr_coattention_bwd(const float* Gu, const float* Gi, const float* M, const float* T, const float* soft_u,
                         const float* soft_i, const float* colmax, const int32_t* argcol, const float* rowmax,
                         const int32_t* argrow, const float* d_atte_u, long ld_du, const float* d_atte_i, long ld_di,
                         const float* d_soft_u, const float* d_soft_i, int B, int SL, float* dGu, float* dGi,
                         float* dM, int accumulate /* add onto dGu,dGi */, float* ws, size_t ws_bytes, void* stream);

/* ---- K6: S-Net (model.py:71-81) ------------------------------------------------------------------------------
 * X [B][S][L][128]; Ms [64][128]; Ws [64]; word_soft [B][S][wl] (wl = L for soft_u/soft_i, V for view_p).
 * Outputs: self_atte [B][S][128], senti rows at senti + b*ld_senti.  Saved: U [B][S][L][64], P [B][S][L], wsum [B][S]. */
int umpr_snet_fwd(const float* X, const float* Ms, const float* Ws, const float* word_soft, int wl, int B, int S,
                  int L, float* U, float* P, float* wsum, float* self_atte, float* senti, long ld_senti, void* stream);
/* umpr_snet_fwd with valid [B][S][L] bytes: P is the softmax of the word scores over the valid tokens of a sentence and +0.0 at
 * the others; a sentence without a valid token gets P = 0 and self_atte = 0.  wsum and senti keep their formulas.  umpr_snet_bwd
 * reads P and needs no mask. */
int umpr_snet_fwd_masked(const float* X, const float* Ms, const float* Ws, const float* word_soft, int wl, int B, int S,
                         int L, float* U, float* P, float* wsum, float* self_atte, float* senti, long ld_senti,
                         const uint8_t* valid, void* stream);
size_t umpr_snet_bwd_ws_bytes(int B, int S, int L);
int umpr_snet_bwd(const float* X, const float* Ms, const float* Ws, const float* U, const float* P, const float* wsum,
                  const float* self_atte, const float* d_senti, long ld_ds, const float* d_self_atte /*or NULL*/,
                  int B, int S, int L, int wl, float* dX, float* dMs, float* dWs, float* d_word_soft /*or NULL*/,
                  float* ws, size_t ws_bytes, void* stream);

/* ---- K7: ReviewNet merge tanh(W_u [atte_u;senti_u] + W_i [atte_i;senti_i]) (model.py:166-168) ----------------
 * repr_u, repr_i [B][256]; W_u, W_i [128][256]; out [B][128]. */
int umpr_review_merge_fwd(const float* repr_u, const float* repr_i, const float* W_u, const float* W_i, int B,
                          float* out, void* stream);
size_t umpr_review_merge_bwd_ws_bytes(int B);
int umpr_review_merge_bwd(const float* repr_u, const float* repr_i, const float* W_u, const float* W_i,
                          const float* out, const float* d_out, int B, float* d_repr_u, float* d_repr_i, float* dW_u,
                          float* dW_i, float* ws, size_t ws_bytes, void* stream);

/* ---- K8: C-Net head: Conv1d(128->KC,k=KS,pad)+ReLU+max_L, Linear(KC->V)+Sigmoid, threshold, sum p^2
 * (model.py:118-125).  X [B][S][L][128]; Wc [KC][128][KS]; Wl [V][KC].  Outputs view_p [B][S][V], final [B][V].
 * Saved: Y [B][S][L][KC], cmax [B][S][KC], argl int32 [B][S][KC], sp [B][S][V].
 * The maximum runs over the Lout = L + 2 ((KS-1)/2) - KS + 1 valid positions of nn.Conv1d(padding=(KS-1)/2): L for an odd KS, L - 1
 * for an even one (Y holds L positions; for an even KS the last one reads a zero past the sentence and never wins).  argl is the
 * FIRST position that attains the maximum (strict `>` while scanning l = 0 .. Lout-1): past a sentence's length the GRU output
 * is zero, every all-zero window gives exactly relu(bc[k]), and of such bit-equal positions the lowest index receives the
 * gradient.  view_p = sp < thr ? 0 : sp (an sp equal to thr is kept).
 * Limits: KS >= 1, Lout >= 1, KC <= 512; the backward also needs KC % 4 == 0 and (4 V KC + 8 V) * 4 bytes <= 65536 (the LDS its
 * head kernel requests, i.e. V (KC + 2) <= 4096: V <= 7 at KC = 512).  The backward checks every argument before its first
 * launch or memset: a refused call writes nothing, whatever the accumulate flags. */
size_t umpr_cnet_head_fwd_ws_bytes(int B, int S, int L, int KS);
int umpr_cnet_head_fwd(const float* X, const float* Wc, const float* bc, const float* Wl, const float* bl, float thr,
                       int B, int S, int L, int KC, int KS, int V, float* Y, float* cmax, int32_t* argl, float* sp,
                       float* view_p, float* final_, float* ws, size_t ws_bytes, void* stream);
/* umpr_cnet_head_fwd with a key-padding mask: valid [B][S][L] bytes as umpr_token_mask writes them.  n_s of a
 * sentence is the length of its LEADING run of valid bytes (a hole ends the run: valid, invalid, valid gives n_s = 1; for what the
 * loader produces n_s is the number of valid tokens).  Y is computed as above; cmax[k] / argl[k] run over the conv positions
 * l < lout = n_s for an odd KS, n_s - 1 for an even one (nn.Conv1d(padding=(KS-1)/2) on n_s tokens), first position on ties.  A
 * sentence with lout < 1 - a padded sentence, or one token under an even KS - is undefined: cmax = +0.0, argl = -1, sp = +0.0,
 * view_p = +0.0 for every k and v, and it adds exactly +0.0 to final; a sample without a defined sentence gets final = 0.  With
 * every byte set each output has the bits of umpr_cnet_head_fwd.  Same outputs, saved tensors, launches and workspace size;
 * umpr_cnet_head_bwd consumes them unchanged (it multiplies by view_p > 0 and writes dY only behind cmax > 0, so argl = -1 forms
 * no address and an undefined sentence's gradients are +0.0).  A NULL mask is refused before any launch. */
int umpr_cnet_head_fwd_masked(const float* X, const float* Wc, const float* bc, const float* Wl, const float* bl, float thr,
                              int B, int S, int L, int KC, int KS, int V, float* Y, float* cmax, int32_t* argl, float* sp,
                              float* view_p, float* final_, const uint8_t* valid, float* ws, size_t ws_bytes, void* stream);
size_t umpr_cnet_head_bwd_ws_bytes(int B, int S, int L, int KC, int KS, int V);
int umpr_cnet_head_bwd(const float* X, const float* Wc, const float* Wl, const float* cmax, const int32_t* argl,
                       const float* sp, const float* view_p, const float* d_final /*or NULL*/,
                       const float* d_view_p /*or NULL*/, int B, int S, int L, int KC, int KS, int V, float* dX,
                       int accumulate_dX, int accumulate_w /* add onto dX / the weight grads */, float* dWc,
                       float* dbc, float* dWl, float* dbl, float* ws, size_t ws_bytes, void* stream);

/* ---- K9: control gate incl. SS-Net (model.py:142-143,186-197) ------------------------------------------------ */
int umpr_control_gate_fwd(const float* self_atte, const float* w, const float* bias, const float* view_p,
                          const float* c_out, int B, int S, int V, float* senti, float* view_score,
                          float* prefer_pos, float* prefer_neg, void* stream);
size_t umpr_control_gate_bwd_ws_bytes(int B);
int umpr_control_gate_bwd(const float* self_atte, const float* w, const float* view_p, const float* c_out,
                          const float* senti, const float* view_score, const float* d_prefer_pos,
                          const float* d_prefer_neg, int B, int S, int V, float* d_self_atte, float* d_view_p,
                          float* d_c_out, float* dw, float* db, float* ws, size_t ws_bytes, void* stream);

/* ---- the text path in two calls per direction (round 3; csrc/text_path.hip) -----------------------------------------------
 * The whole ReviewNet (src/model.py:157-169: R-Net GRU over the user + item pair, co-attention, S-Net u / i, merge) and the whole
 * ControlNet (src/model.py:179-198: C-Net GRU over ui and over the pair, three C-Net heads, control S-Net, SS-Net gate), each
 * issued back to back from C++ into ONE caller-owned arena (everything the backward reads; *_arena_bytes) and one scratch buffer
 * (*_ws_bytes).  Same kernels and the same arithmetic as the per-stage entry points above, which these call in order; what goes
 * away is ~20 host round trips per direction (a UMPR-R training step is 0.9 ms of kernels).
 * ids_pair [2N][L]: user rows then item rows (umpr_concat_ids); lengths / order [2N] with the item half's order offset by N.
 * b16_gemm: GEMM-shaped products on the bf16 pipe (as umpr_set_gemm_bf16); b16_scores: the co-attention score contraction in
 * bf16 (as umpr_coattention_fwd_bf16); need_grad = 0 skips the GRU gate records (inference). */
int umpr_concat_ids(const int64_t* ids_u, const int64_t* ids_i, long n_each, int64_t* dst, void* stream);
size_t umpr_review_net_arena_bytes(int B, int S, int L);
size_t umpr_review_net_ws_bytes(int B, int S, int L, int E);
/* params (15): w_ih_f, w_hh_f, b_ih_f, b_hh_f, w_ih_r, w_hh_r, b_ih_r, b_hh_r, M, Ms_u, Ws_u, Ms_i, Ws_i, W_u, W_i; out [B][128] */
int umpr_review_net_fwd(const int64_t* ids_pair, const float* emb, int E, const float* const* params, const int32_t* lengths,
                        const int32_t* order, int B, int S, int L, int b16_gemm, int b16_scores, int need_grad, void* arena,
                        float* out, float* ws, size_t ws_bytes, void* stream);
/* The same through umpr_coattention_fwd_masked and umpr_snet_fwd_masked: valid_pair [2N][L] bytes, user rows then item rows, as
 * umpr_token_mask writes them for ids_pair.  Same arena, same workspace; both backward calls read the arena as they do. */
int umpr_review_net_fwd_masked(const int64_t* ids_pair, const float* emb, int E, const float* const* params,
                               const int32_t* lengths, const int32_t* order, int B, int S, int L, int b16_gemm, int b16_scores,
                               int need_grad, void* arena, float* out, float* ws, size_t ws_bytes, const uint8_t* valid_pair,
                               void* stream);
/* grads: 15 pointers in the order of params, each overwritten */
int umpr_review_net_bwd(const int64_t* ids_pair, const float* emb, int E, const float* const* params, const int32_t* lengths,
                        const int32_t* order, int B, int S, int L, int b16_gemm, const void* arena, const float* d_out,
                        float* const* grads, float* ws, size_t ws_bytes, void* stream);
/* umpr_review_net_bwd that also hands out the token gradient of the user+item pair, dx_pair [2N*L][E] (overwritten; see
 * umpr_embed_gru_bidir_bwd_dx).  dx_pair = NULL is umpr_review_net_bwd.  Same workspace. */
int umpr_review_net_bwd_dx(const int64_t* ids_pair, const float* emb, int E, const float* const* params, const int32_t* lengths,
                           const int32_t* order, int B, int S, int L, int b16_gemm, const void* arena, const float* d_out,
                           float* const* grads, float* dx_pair, float* ws, size_t ws_bytes, void* stream);
/* The general forms of the three ReviewNet calls above.  dst_row [2N]: the output row of each input row of the pair in the R-Net
 * GRU (umpr_embed_gru_bidir_fwd): `order` is the reference's double un-sort (what the calls above pass), the identity 0..2N-1 lets
 * every sentence keep its own states (--unsort_gru); `order` then only groups similar lengths into tiles.  The backward takes the
 * dst_row of its forward.  valid_pair and dx_pair may each be NULL.  Same arena, same workspace; dst_row and valid_pair are the
 * caller's buffers. */
int umpr_review_net_fwd_ex(const int64_t* ids_pair, const float* emb, int E, const float* const* params, const int32_t* lengths,
                           const int32_t* order, const int32_t* dst_row, int B, int S, int L, int b16_gemm, int b16_scores,
                           int need_grad, void* arena, float* out, float* ws, size_t ws_bytes, const uint8_t* valid_pair /*or NULL*/,
                           void* stream);
int umpr_review_net_bwd_ex(const int64_t* ids_pair, const float* emb, int E, const float* const* params, const int32_t* lengths,
                           const int32_t* order, const int32_t* dst_row, int B, int S, int L, int b16_gemm, const void* arena,
                           const float* d_out, float* const* grads, float* dx_pair /*or NULL*/, float* ws, size_t ws_bytes,
                           void* stream);
size_t umpr_control_net_arena_bytes(int B, int S_ui, int L_ui, int S, int L, int KC, int V);
size_t umpr_control_net_ws_bytes(int B, int S_ui, int L_ui, int S, int L, int E, int KC, int KS, int V);
/* params (16): the C-Net GRU's eight, Wc [KC][128][KS], bc, Wl [V][KC], bl, Ms, Ws, ssW [128], ssb [1];
 * outputs c_u, c_i, prefer_pos, prefer_neg [B][V] */
int umpr_control_net_fwd(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* params,
                         const int32_t* len_ui, const int32_t* ord_ui, const int32_t* len_pair, const int32_t* ord_pair, int B,
                         int S_ui, int L_ui, int S, int L, int KC, int KS, int V, float thr, int b16_gemm, int need_grad, void* arena,
                         float* c_u, float* c_i, float* prefer_pos, float* prefer_neg, float* ws, size_t ws_bytes, void* stream);
int umpr_control_net_bwd(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* params,
                         const int32_t* len_ui, const int32_t* ord_ui, const int32_t* len_pair, const int32_t* ord_pair, int B,
                         int S_ui, int L_ui, int S, int L, int KC, int KS, int V, int b16_gemm, const void* arena, const float* d_cu,
                         const float* d_ci, const float* d_pp, const float* d_pn, float* const* grads, float* ws, size_t ws_bytes,
                         void* stream);
/* umpr_control_net_bwd that also hands out the token gradients of the C-Net GRU's two calls: dx_pair [2N*L][E] and
 * dx_ui [B*S_ui*L_ui][E] (each overwritten; both NULL is umpr_control_net_bwd, one NULL is refused).  Same workspace. */
int umpr_control_net_bwd_dx(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* params,
                            const int32_t* len_ui, const int32_t* ord_ui, const int32_t* len_pair, const int32_t* ord_pair, int B,
                            int S_ui, int L_ui, int S, int L, int KC, int KS, int V, int b16_gemm, const void* arena, const float* d_cu,
                            const float* d_ci, const float* d_pp, const float* d_pn, float* const* grads, float* dx_pair,
                            float* dx_ui, float* ws, size_t ws_bytes, void* stream);

/* The general forms of the ControlNet calls: dst_ui [B*S_ui] / dst_pair [2N] as dst_row above for the C-Net GRU's two calls, and
 * valid_ui [B*S_ui][L_ui] / valid_pair [2N][L] (both or neither; one NULL is refused before any launch): with them the three heads
 * run as umpr_cnet_head_fwd_masked and the control S-Net as umpr_snet_fwd_masked on valid_ui (--mask_control).  The gate and the
 * backward need no mask: every term they form carries a factor view_p, +0.0 for an undefined sentence.  dx_pair / dx_ui: both or
 * neither, as umpr_control_net_bwd_dx.  Same arena, same workspace. */
int umpr_control_net_fwd_ex(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* params,
                            const int32_t* len_ui, const int32_t* ord_ui, const int32_t* dst_ui, const int32_t* len_pair,
                            const int32_t* ord_pair, const int32_t* dst_pair, int B, int S_ui, int L_ui, int S, int L, int KC, int KS,
                            int V, float thr, int b16_gemm, int need_grad, void* arena, float* c_u, float* c_i, float* prefer_pos,
                            float* prefer_neg, float* ws, size_t ws_bytes, const uint8_t* valid_ui, const uint8_t* valid_pair,
                            void* stream);
int umpr_control_net_bwd_ex(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* params,
                            const int32_t* len_ui, const int32_t* ord_ui, const int32_t* dst_ui, const int32_t* len_pair,
                            const int32_t* ord_pair, const int32_t* dst_pair, int B, int S_ui, int L_ui, int S, int L, int KC, int KS,
                            int V, int b16_gemm, const void* arena, const float* d_cu, const float* d_ci, const float* d_pp,
                            const float* d_pn, float* const* grads, float* dx_pair, float* dx_ui, float* ws, size_t ws_bytes,
                            void* stream);

/* ---- K10: VGG16-D feature extractor (torchvision.models.vgg16, call site model.py:204-207,217) ---------------
 * images [n][3][224][224]; params: 32 pointers = 13 x (conv weight [Cout][Cin][3][3], bias) then 3 x (fc weight
 * [out][in], bias) in torchvision order.  acts: activation arena (umpr_vgg16_act_bytes), kept for backward.
 * train!=0 applies Dropout(0.5) after fc1/fc2 with a counter-hash mask from `seed`; use_masks!=0 reads the caller's
 * keep-masks (uint8 [2][n][4096] in `masks`) instead (parity tests).  out [n][1000].
 * Generated masks are bytes 0 / 1 and a pure function of (seed, layer, element index): layer j hashes the element index
 * row * 4096 + column with seed + (j + 1) * 0x9E3779B97F4A7C15, so a row's mask does not depend on n_img and the same seed
 * gives the same bytes.  Injected masks are read only.  A call writes every byte it uses: the classifier forward all of out,
 * the fc1 / fc2 regions of the arena and - when dropout runs - the two dropout regions and, when it generates them, the masks
 * (in eval mode the dropout regions and the masks are not touched); the backward all six classifier gradients and d_pool5;
 * neither reads workspace bytes it has not written itself.  The three classifier backwards (umpr_vgg16_classifier_bwd,
 * _bwd_compact, _bwd_compact_bf16) take d_pool5 == NULL for a caller whose convolutional stage does not train: the six
 * gradients are written exactly as with a d_pool5, fc1's data-gradient product (a second pass over its 411 MB matrix) is
 * not launched and nothing of size n x 25088 is written; the workspace size is the same.  n_img < 1 and a workspace below the queried size are refused
 * before anything is launched.  Above 128 images the classifier's products run on the generic GEMM above (in its bf16 mode
 * under the _bf16 entry points). */
size_t umpr_vgg16_act_bytes(int n_img);
size_t umpr_vgg16_fwd_ws_bytes(int n_img);
size_t umpr_vgg16_ws_bytes(int n_img); /* backward workspace */
int umpr_vgg16_fwd(const float* images, const float* const* params, int n_img, int train, int use_masks,
                   uint64_t seed, float* acts, uint8_t* masks, float* out, float* ws, size_t ws_bytes, void* stream);
/* grads: 32 pointers matching params (overwritten).  train != 0 <=> dropout was applied in the forward pass
 * (train or use_masks). */
int umpr_vgg16_bwd(const float* images, const float* const* params, int n_img, int train, const float* acts,
                   const uint8_t* masks, const float* d_out, float* const* grads, float* ws, size_t ws_bytes,
                   void* stream);
/* The same in two stages, so that a host can start exchanging the classifier gradients (89 % of all gradient bytes:
 * fc1 alone is 411 MB) while the convolutional backward still runs.  pool5 = acts + umpr_vgg16_pool5_offset(n) bytes
 * is the [n][512][7][7] output of the feature stage; d_pool5 [n][25088]. */
size_t umpr_vgg16_pool5_offset(int n_img);
int umpr_vgg16_features_fwd(const float* images, const float* const* params, int n_img, float* acts, float* ws,
                            size_t ws_bytes, void* stream);
int umpr_vgg16_classifier_fwd(const float* const* params, int n_img, int train, int use_masks, uint64_t seed,
                              float* acts, uint8_t* masks, float* out, float* ws, size_t ws_bytes, void* stream);
size_t umpr_vgg16_classifier_bwd_ws_bytes(int n_img);
int umpr_vgg16_classifier_bwd(const float* const* params, int n_img, int train, const float* acts,
                              const uint8_t* masks, const float* d_out, float* const* grads, float* d_pool5, float* ws,
                              size_t ws_bytes, void* stream);
size_t umpr_vgg16_features_bwd_ws_bytes(int n_img);
int umpr_vgg16_features_bwd(const float* images, const float* const* params, int n_img, const float* acts,
                            const float* d_pool5, float* const* grads, float* ws, size_t ws_bytes, void* stream);
/* Data parallel: `cb(block, user)` is called on the calling thread each time umpr_vgg16_features_bwd /
 * umpr_vgg16_bf16_features_bwd has ENQUEUED all kernels of one VGG block (4, 3, 2, 1, 0), i.e. as soon as that block's
 * weight gradients are ordered on umpr_vgg16_wgrad_stream() (the library's side stream; NULL when weight gradients run on
 * the caller's stream).  A host that owns flat gradient storage starts that block's all-reduce there, ordered behind that
 * stream, while the blocks below are still being computed.  cb = NULL clears it. */
typedef void (*umpr_block_callback)(int block, void* user);
int umpr_vgg16_set_block_callback(umpr_block_callback cb, void* user);
void* umpr_vgg16_wgrad_stream(void);
/* per-layer entry points (also what the composite calls) */
/* Any N, Cin, Cout, H, W >= 1; maps need not be square (only the square 224/112/56/28/14 maps have kernels of their own, any
 * other map - non-square, one pixel high or wide - runs the generic kernels at the same accuracy).
 * wpack / wt: scratch of umpr_conv3x3_pack_bytes(...) - packed weights, or on the 56/28/14 maps (and 112 with >= 128 channels)
 * the Winograd buffers.  Nothing is read from it that the call did not write, nothing is written behind its size, and the
 * result does not depend on it being larger.  With less:
 *   - a layer planned on Winograd runs the direct kernel as long as the packed weights fit - Cout * ceil(Cin / 4) * 36 floats in
 *     forward, Cin * ceil(Cout / 4) * 36 in the data gradient; below that the call is refused ("weight scratch too small") and
 *     writes nothing;
 *   - umpr_conv3x3_fwd with wpack = NULL, wpack_bytes = 0 runs the generic kernel on every shape; umpr_conv3x3_bwd_data needs
 *     its scratch and refuses NULL ("needs the weight scratch");
 *   - umpr_conv3x3_bwd_weight with k * (9 * Cout * Cin + Cout) * 4 bytes, k >= 1 below what umpr_conv3x3_bwd_weight_ws_bytes
 *     reports, runs the shape's non-Winograd kernel with at most k split-K slabs ([9][Cout][Cin] each, the bias rows behind
 *     them); less than one slab is refused ("workspace too small") with nothing written.
 * (tests/test_gpu_conv_seams.py pins all of this on NaN-filled buffers between guard bands.) */
size_t umpr_conv3x3_pack_bytes(int N, int Cin, int Cout, int H, int W);
int umpr_conv3x3_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int H, int W,
                     int Cout, int relu, float* wpack, size_t wpack_bytes, void* stream);
/* dx = conv_transpose(dy, w) [* (mask_src > 0)].  The comparison is IEEE's and flushes nothing: false at +0, -0 and every
 * negative value, true at positive denormals.  Where it is true dx holds the bits of the unmasked call, elsewhere +0. */
int umpr_conv3x3_bwd_data(const float* dy, const float* w, const float* mask_src /*or NULL*/, float* dx, int N,
                          int Cin, int H, int W, int Cout, float* wt, size_t wt_bytes, void* stream);
size_t umpr_conv3x3_bwd_weight_ws_bytes(int N, int Cin, int Cout, int H, int W);
int umpr_conv3x3_bwd_weight(const float* dy, const float* x, float* dw, float* db, int N, int Cin, int H, int W,
                            int Cout, float* ws, size_t ws_bytes, void* stream);
int umpr_maxpool2_fwd(const float* x, float* y, long planes, int H, int W, void* stream);
int umpr_maxpool2_bwd_relu(const float* x, const float* dy, float* dx, long planes, int H, int W, void* stream);

/* ---- bf16 mixed precision (BASELINE.json configs[4]: "MFMA bf16 conv + attention; MSE within 1e-3 of fp32") ---------
 * Replaces the same torchvision VGG16 call site (model.py:204-207,217) with bf16 activations / gradients, fp32
 * accumulation and fp32 master weights: v_mfma_f32_32x32x16_bf16 implicit GEMM.  Activations live in the library's
 * CB8-PF layout (umpr_amd/csrc/bf16_conv.hip: channel blocks of 8, padded-flat pixels with zero borders); a tensor of
 * N x C x H x W takes umpr_bf16_tensor_bytes(...) bytes and is produced / read back by the two converters.  Per-layer
 * entry points (parity tests): channels must be multiples of 64 (32 for a reduction), maps 224/112/56/28/14 square.
 * ws: umpr_conv3x3_bf16_ws_bytes(...) bytes of scratch (packed bf16 weights, or split-K slabs of the weight gradient): the
 * largest of what the three passes need for the shape, rounded up to 1024.  Per pass the least a call accepts is
 *   - forward and data gradient: Cin * Cout * 18 + 1024 bytes (the packed bf16 weights), below that "weight scratch too small";
 *   - weight gradient: splits * (9 * Cout * Cin + Cout) * 4 + 1024 bytes (one fp32 slab [Cout][Cin][9] and one bias row per
 *     split), below that "workspace too small"; `splits` is what umpr_debug_conv_bf16_plan reports for the shape.
 * Forward takes Cin % 32 == 0 and Cout % 64 == 0, the data gradient Cout % 32 == 0 and Cin % 64 == 0, the weight gradient both
 * % 64 == 0; for a shape a pass refuses, umpr_conv3x3_bf16_ws_bytes covers the passes that take it.  The three conv entry points
 * and the two pools require N, Cin, Cout (C), H, W > 0 and every pointer but bias, mask_src and db non-NULL; a call that fails a
 * check names the cause in umpr_last_error, returns non-zero, and has launched and written nothing.  Nothing is read from ws
 * that the call did not write, and the result does not depend on it being larger (tests/test_gpu_bf16_conv_seams.py). */
size_t umpr_bf16_tensor_bytes(int N, int C, int H, int W);
int umpr_bf16_from_nchw_f32(const float* x, void* y, int N, int C, int H, int W, void* stream);
int umpr_bf16_to_nchw_f32(const void* x, float* y, int N, int C, int H, int W, void* stream);
size_t umpr_conv3x3_bf16_ws_bytes(int N, int Cin, int Cout, int H, int W);
int umpr_conv3x3_bf16_fwd(const void* x, const float* w, const float* bias, void* y, int N, int Cin, int H, int W,
                          int Cout, int relu, void* ws, size_t ws_bytes, void* stream);
/* dx = conv_transpose(dy, w) [* (mask_src > 0)], mask_src in the same layout as dx.  The comparison is the fp32 entry point's:
 * IEEE's, nothing flushed - false at +0, -0 and every negative value, true at positive bf16 subnormals.  Where it is true dx
 * holds the bits of the unmasked call, elsewhere +0. */
int umpr_conv3x3_bf16_bwd_data(const void* dy, const float* w, const void* mask_src /*or NULL*/, void* dx, int N,
                               int Cin, int H, int W, int Cout, void* ws, size_t ws_bytes, void* stream);
/* dw [Cout][Cin][3][3], db [Cout] in fp32 (overwritten) */
int umpr_conv3x3_bf16_bwd_weight(const void* dy, const void* x, float* dw, float* db, int N, int Cin, int H, int W,
                                 int Cout, void* ws, size_t ws_bytes, void* stream);
int umpr_maxpool2_bf16_fwd(const void* x, void* y, int N, int C, int H, int W, void* stream);
int umpr_maxpool2_bf16_bwd_relu(const void* x, const void* dy, void* dx, int N, int C, int H, int W, void* stream);
/* The convolutional stage of VGG16 in bf16.  images fp32 [n][3][224][224]; params / grads: the same 32-pointer fp32
 * tables as umpr_vgg16_features_*; acts: umpr_vgg16_bf16_act_bytes(n) bytes kept for backward; pool5 / d_pool5: fp32
 * [n][25088] in NCHW flatten order (what the classifier consumes / produces). */
size_t umpr_vgg16_bf16_act_bytes(int n_img);
size_t umpr_vgg16_bf16_fwd_ws_bytes(int n_img);
size_t umpr_vgg16_bf16_bwd_ws_bytes(int n_img);
int umpr_vgg16_bf16_features_fwd(const float* images, const float* const* params, int n_img, void* acts, float* pool5,
                                 void* ws, size_t ws_bytes, void* stream);
int umpr_vgg16_bf16_features_bwd(const float* images, const float* const* params, int n_img, const void* acts,
                                 const float* d_pool5, float* const* grads, void* ws, size_t ws_bytes, void* stream);
/* The classifier on a compact fp32 arena of umpr_vgg16_cls_arena_bytes(n): [pool5 n x 25088][fc1, fc2 ReLU outputs]
 * [their dropout outputs] - for callers whose feature stage does not use the fp32 activation arena (the bf16 path).
 * Workspaces as for umpr_vgg16_classifier_fwd / _bwd. */
size_t umpr_vgg16_cls_arena_bytes(int n_img);
int umpr_vgg16_classifier_fwd_compact(const float* const* params, int n_img, int train, int use_masks, uint64_t seed,
                                      float* cls_arena, uint8_t* masks, float* out, float* ws, size_t ws_bytes,
                                      void* stream);
int umpr_vgg16_classifier_bwd_compact(const float* const* params, int n_img, int train, const float* cls_arena,
                                      const uint8_t* masks, const float* d_out, float* const* grads, float* d_pool5,
                                      float* ws, size_t ws_bytes, void* stream);
/* The same under mixed precision (torch.autocast would run these nn.Linear layers in bf16 too): operands rounded to
 * bf16 in registers, v_mfma_f32_32x32x16_bf16 with fp32 accumulation; everything in memory stays fp32. */
int umpr_vgg16_classifier_fwd_compact_bf16(const float* const* params, int n_img, int train, int use_masks,
                                           uint64_t seed, float* cls_arena, uint8_t* masks, float* out, float* ws,
                                           size_t ws_bytes, void* stream);
int umpr_vgg16_classifier_bwd_compact_bf16(const float* const* params, int n_img, int train, const float* cls_arena,
                                           const uint8_t* masks, const float* d_out, float* const* grads,
                                           float* d_pool5, float* ws, size_t ws_bytes, void* stream);

/* ---- K11-K12: visual head + fusion + losses (model.py:218-228,267-277) ----------------------------------------
 * V = 0 selects the review_net_only branch (model.py:267-269).  loss [3] = (loss, loss_r, loss_v). */
int umpr_head_fwd(const float* rr, const float* c_u, const float* c_i, const float* prefer_pos,
                  const float* prefer_neg, const float* vgg, const float* pos_v_emb, const float* neg_v_emb,
                  const float* lin_w, const float* lin_b, const float* fus_w, const float* fus_b, const float* labels,
                  float loss_v_rate, int B, int V, int P, float* pred, float* loss, float* z, float* img_emb,
                  float* pos_match, float* neg_match, float* posneg_emb, void* stream);
int umpr_head_bwd(const float* rr, const float* c_u, const float* c_i, const float* prefer_pos,
                  const float* prefer_neg, const float* vgg, const float* pos_v_emb, const float* neg_v_emb,
                  const float* lin_w, const float* fus_w, const float* labels, float loss_v_rate, int B, int V, int P,
                  const float* pred, const float* z, const float* img_emb, const float* pos_match,
                  const float* neg_match, const float* posneg_emb, const float* d_loss, const float* d_pred /*or NULL*/,
                  float* d_rr, float* d_cu, float* d_ci, float* d_pp, float* d_pn, float* d_vgg, float* d_pos_v,
                  float* d_neg_v, float* d_lin_w, float* d_lin_b, float* d_fus_w, float* d_fus_b, void* stream);

/* ---- photo resize (umpr_amd/photos.py; finishes src/dataset.py:134-143's get_image on the device) ----------------------------
 * The loader decodes each photo on the host and ships, in ONE uint8 buffer `packed` of `packed_bytes` (device memory), only the
 * source rows and columns its resize taps read, plus per-photo tap tables it computed with the numpy expressions of
 * umpr_amd/data.py::resize_bilinear_u8.  out [n_photos][3][dst_h][dst_w] fp32 = that resize (OpenCV's 8-bit INTER_LINEAR,
 * 11-bit fixed point) / 255, bit-identical to the host path.  `desc` is HOST memory (n_photos entries, read and validated during
 * the call: every region must lie inside the buffer, else the call fails without launching); offsets are bytes into `packed`.
 * Tap tables, int32 at desc.taps (4-byte aligned): cx0[dst_w] cx1[dst_w] ax0[dst_w] ax1[dst_w] ry0[dst_h] ry1[dst_h] by0[dst_h]
 * by1[dst_h] - column / row indices into the compacted source and their weights.  rows = cols = 0 marks a missing photo
 * (all-zero image).  No allocation or copy: capture-safe. */
typedef struct umpr_photo_desc {
  int64_t pixels; /* byte offset of the compacted source, uint8 [rows][cols][3] (RGB) */
  int64_t taps;   /* byte offset of the tap tables */
  int32_t rows;
  int32_t cols;
} umpr_photo_desc;
int umpr_photo_resize_u8(const uint8_t* packed, size_t packed_bytes, const umpr_photo_desc* desc, int n_photos, int dst_h,
                         int dst_w, float* out, void* stream);

/* ---- device-resident photo store (umpr_amd/photos.py::PhotoStore) ---------------------------------------------------------------
 * `store` (device memory, 16-byte aligned) holds n_slots slots of umpr_photo_store_slot_bytes(dst_h, dst_w) bytes: the uint8 value
 * behind every output pixel of one resized photo, planar [3][dst_h][dst_w] (slot byte j <-> output float j), so that
 * out = lut[slot] reproduces umpr_photo_resize_u8's floats bit for bit.  src_slot, dst_slot and desc are HOST memory (n_photos
 * entries each), read and validated during the call.  Photo i with src_slot[i] >= 0 is read from that slot (its descriptor must
 * be 0 x 0); otherwise it is resized exactly as by umpr_photo_resize_u8 (zeros for a 0 x 0 descriptor) and, if dst_slot[i] >= 0,
 * its uint8 image is also written to that slot.  Refused without launching: a slot outside [0, n_slots), a null store with a slot
 * in use, a hit with a non-empty descriptor, a dst_slot on a 0 x 0 descriptor, one dst_slot given twice, a dst_slot that a photo
 * of the same call reads.  No allocation or copy: capture-safe. */
size_t umpr_photo_store_slot_bytes(int dst_h, int dst_w); /* 3*dst_h*dst_w rounded up to 16; 0 for a size the resize refuses */
int umpr_photo_fetch_u8(const uint8_t* packed, size_t packed_bytes, const umpr_photo_desc* desc, const int32_t* src_slot,
                        const int32_t* dst_slot, int n_photos, int dst_h, int dst_w, uint8_t* store, long n_slots, float* out,
                        void* stream);

/* ---- augmented photo fetch (umpr_amd/photos.py::PhotoAugment): random crop and flip at the fetch -------------------------------
 * umpr_photo_fetch_u8 with a window and a flip per photo.  With U [dst_h][dst_w][3] the resized uint8 image of photo i (what a
 * slot holds planar) and crop[i] = (x0, y0, cw, ch, flip), HOST int32 [n_photos][5]:
 *   A = resize_bilinear_u8(U[y0:y0+ch, x0:x0+cw], (dst_w, dst_h));  A = A[:, ::-1] if flip;  out[i] = lut[A] planar,
 * bit for bit; a 0 x 0 descriptor without a src_slot gives zeros whatever its record says; (0, 0, dst_w, dst_h, 0) is
 * umpr_photo_fetch_u8's photo.  A decoded photo is first resized exactly as there, uint8 only: into its dst_slot when it has one -
 * a store slot always receives the plain image - else into the next free slot of `scratch` (device, 16-byte aligned, n_scratch
 * slots of umpr_photo_store_slot_bytes).  Then one kernel writes `out` for the whole chunk from store and scratch, on the same
 * stream.  store == NULL with n_slots == 0: everything goes through scratch.  xtaps [dst_w][4][dst_w] and ytaps [dst_h][4][dst_h]
 * (device int32) hold, in row s-1, the concatenated data._column_taps(dst_w, s) / data._row_taps(dst_h, s); the kernel clamps
 * their indices into the window.  Refused without launching, `out`, `store` and `scratch` untouched: all that umpr_photo_fetch_u8
 * refuses; a window outside the image or with cw < 1 or ch < 1; a flip outside {0, 1}; fewer scratch slots than decoded photos
 * without a dst_slot; a null table; scratch or out not 16-byte aligned; dst_h or dst_w above 4096 (the kernel stages the source
 * of an output tile in LDS, and its bound on that source is proven for such sides).  No allocation or copy: capture-safe. */
int umpr_photo_fetch_augment_u8(const uint8_t* packed, size_t packed_bytes, const umpr_photo_desc* desc, const int32_t* src_slot,
                                const int32_t* dst_slot, const int32_t* crop, int n_photos, int dst_h, int dst_w, uint8_t* store,
                                long n_slots, uint8_t* scratch, long n_scratch, const int32_t* xtaps, const int32_t* ytaps,
                                float* out, void* stream);

/* ---- device-resident VGG features (umpr_amd/photos.py::FeatureStore) -----------------------------------------------------------
 * With a frozen VGG (--freeze_vgg) the F floats the stack yields for a photo are a constant of the run.  `store` (device memory)
 * holds n_slots rows of F fp32; `fresh` [n_fresh][F] holds the rows the VGG has just computed for the photos the store lacks.
 * out [n][F]: row i = store[src_slot[i]] if src_slot[i] >= 0, else fresh[fresh_row[i]] (several photos may name one fresh row: the
 * same photo twice in a batch); if dst_slot[i] >= 0 the same row is also written to store[dst_slot[i]].  A bit-exact copy in
 * 16-byte groups.  fresh_row, src_slot and dst_slot are HOST memory (n entries each), read and validated during the call and
 * carried in the kernel arguments, 64 photos per launch.  Refused without launching, `out` and `store` untouched: a slot outside
 * [0, n_slots), a photo with both or neither of src_slot / fresh_row, a fresh_row outside [0, n_fresh), one dst_slot given twice,
 * a dst_slot that a photo of the same call reads, a null store with a slot in use, F not a positive multiple of 4, fresh / store /
 * out not 16-byte aligned.  No allocation or copy: capture-safe. */
int umpr_feature_fetch_f32(const float* fresh, int n_fresh, const int32_t* fresh_row, const int32_t* src_slot,
                           const int32_t* dst_slot, int n, int F, float* store, long n_slots, float* out, void* stream);

/* ---- device-resident tokenised reviews (umpr_amd/reviews.py::ReviewStore) ------------------------------------------------------
 * The text half of umpr_amd/data.py::batch_loader on the device.  `tokens` [T] holds every distinct sentence of a corpus once,
 * sentence j at tokens[sent_off[j] .. sent_off[j+1]); per role (user, item, ui) sample n owns the sentences
 * sid[ptr[n] .. ptr[n+1]); ratings [n_samples].  All of these are device memory.  `idx` is HOST memory (B sample indices), read
 * and validated during the call and carried in the kernel arguments, 256 per launch: a batch of B <= 256 is one launch for all
 * three roles and the labels.  ids_pair [2][B][S][L] (user half, then item half), ids_ui [B][S_ui][L_ui] (may be NULL with
 * S_ui = L_ui = 0) and labels [B] are written in full, every element once: element [b][s][l] is the token if s is below the
 * sample's sentence count and l below that sentence's length, `pad` otherwise; a count above S or a sentence longer than L is
 * truncated.  A sample named twice gives two identical rows.  Refused without launching, the outputs untouched: a NULL tokens,
 * sent_off, idx, ids_pair, labels or ratings, a NULL table of a role in use, B < 1, S or L < 1, L or L_ui > 256, S_ui / L_ui
 * inconsistent with ids_ui, an index outside [0, n_samples).  No allocation or copy: capture-safe. */
int umpr_review_collate(const int32_t* tokens, const int64_t* sent_off, long n_sent, const int64_t* ptr_u, const int32_t* sid_u,
                        const int64_t* ptr_i, const int32_t* sid_i, const int64_t* ptr_ui, const int32_t* sid_ui,
                        const float* ratings, long n_samples, const int32_t* idx, int B, int S, int L, int S_ui, int L_ui, long pad,
                        int64_t* ids_pair, int64_t* ids_ui, float* labels, void* stream);

/* ---- sampled review collate (umpr_amd/reviews.py::ReviewDraw): a fresh draw of each pool per epoch, word dropout -----------------
 * umpr_review_collate with the user and item tables holding pools of up to 1024 sentences, of which a sample shows `keep`.  With
 * mix64 splitmix64's output function, n the sample's index and role 0 / 1 / 2 for user / item / ui:
 *   role_key = mix64(mix64(seed_epoch_key + n) + role),   key_j = mix64(role_key + j) for the pool's positions j;
 * row s of a user or item holds the sentence whose key has rank s among the pool's (ties to the smaller j), for
 * s < min(keep, pool size), and `pad` beyond; the ui rows are umpr_review_collate's.  With drop_threshold T > 0 the token at (s, l)
 * of any role, l inside the sentence's kept length, becomes `unk` iff
 *   (mix64(mix64(role_key ^ 0xD6E8FEB86659FD93) + ((s << 8) | l)) >> 32) < T;
 * padding stays `pad`.  T = 0 runs the instantiation without the test.  seed_epoch_key = mix64(mix64(seed) + epoch) is formed by
 * the caller; drop_threshold is 32 bits wide, min(floor(p * 2^32), 2^32 - 1) for a dropout rate p.  One workgroup per
 * (sample, role); what it reads from the tables is clipped (pool size to 1024, sentence ids to n_sent, lengths to the row), so a
 * corrupt table gives wrong ids, never an access out of bounds.  Refused without launching, the
 * outputs untouched: all that umpr_review_collate refuses; keep outside [1, 1024]; S > keep; T > 0 with unk < 0.  No allocation
 * or copy: capture-safe. */
int umpr_review_collate_sampled(const int32_t* tokens, const int64_t* sent_off, long n_sent, const int64_t* ptr_u,
                                const int32_t* sid_u, const int64_t* ptr_i, const int32_t* sid_i, const int64_t* ptr_ui,
                                const int32_t* sid_ui, const float* ratings, long n_samples, const int32_t* idx, int B, int S, int L,
                                int S_ui, int L_ui, long pad, int keep, uint64_t seed_epoch_key, unsigned int drop_threshold, long unk,
                                int64_t* ids_pair, int64_t* ids_ui, float* labels, void* stream);

/* ---- R-Net pre-training head (pretrain/pretrain_rnet.py:147-169): result = sigmoid(Linear(K -> 1)(att)),
 * loss = BCELoss(mean)(result, target) with torch's log clamp at -100.  att rows at att + b*ld (K = 256: [atte_u;atte_i]
 * as umpr_coattention_fwd leaves them).  ws: B floats.  Backward follows ATen's binary_cross_entropy_backward
 * (denominator max(p(1-p), 1e-12)); d_result may be NULL, d_loss is a device scalar. */
int umpr_bce_head_fwd(const float* att, long ld, const float* w, const float* b, const float* target, int B, int K,
                      float* result, float* loss, float* ws, size_t ws_bytes, void* stream);
int umpr_bce_head_bwd(const float* att, long ld, const float* w, const float* result, const float* target,
                      const float* d_result /*or NULL*/, const float* d_loss, int B, int K, float* d_att, long ld_d,
                      float* dw, float* db, float* ws, size_t ws_bytes, void* stream);

/* ---- K13: Adam step with coupled L2, as torch.optim.Adam drives it in main.py:22-26,37 ----------------------
 * One flat parameter segment: p,g,m,v [n]; step >= 1; grad_scale multiplies g first (1/world for data parallel). */
int umpr_adam_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                   double eps, double weight_decay, long step, double grad_scale, void* stream);

/* The same step with its per-step scalars in DEVICE memory - hyper[4] = {grad_scale, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t),
 * weight_decay} in the kernel's fp32 - so that a captured hipGraph of a training step can be replayed while t advances: the
 * host refreshes the four floats before each replay (umpr_amd/graphs.py). */
int umpr_adam_step_dev(float* p, const float* g, float* m, float* v, long n, double beta1, double beta2, double eps,
                       const float* hyper, void* stream);

/* ---- Gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, L2) fused into the optimiser step --------------
 * umpr_grad_norm: norm = |grad_scale| * sqrt(sum of squares over every element of the n_arenas flat arrays) and
 * coef = min(1, max_norm / (norm + 1e-6)), both formed in double and rounded once to float.  grads / counts are HOST arrays of
 * n_arenas (<= 8) device pointers / element counts, read during the call; any float-aligned pointer and any count >= 0 are
 * accepted.  The scale is grad_scale_dev[0] (device memory: what a captured graph reads) if that pointer is not NULL, the host
 * value grad_scale otherwise.  Two launches on a fixed grid - squares exact in double, one double partial per workgroup in ws,
 * one workgroup adds the partials in a fixed order - and no atomics: the result is bit-reproducible and does not depend on the
 * device.  No allocation, no copy: capture-safe.  ws: umpr_grad_norm_ws_bytes() bytes of device memory.
 * state: 8 device floats the caller zeroes once; every call writes the first four and advances the counters:
 *   [COEF] the coefficient (0 if the norm is not finite)   [NORM] the norm of the scaled gradient, before clipping
 *   [FINITE] 1.0f / 0.0f                                   [MAX_NORM] max_norm as given
 *   [SEEN] [CLIPPED] [SKIPPED] uint32 counters in the float slots: calls, calls with coef < 1, calls with a non-finite norm. */
enum { UMPR_CLIP_COEF = 0, UMPR_CLIP_NORM = 1, UMPR_CLIP_FINITE = 2, UMPR_CLIP_MAX_NORM = 3, UMPR_CLIP_SEEN = 4,
       UMPR_CLIP_CLIPPED = 5, UMPR_CLIP_SKIPPED = 6 };
size_t umpr_grad_norm_ws_bytes(void);
int umpr_grad_norm(const float* const* grads, const long* counts, int n_arenas, double max_norm, float grad_scale,
                   const float* grad_scale_dev /*or NULL*/, double* ws, size_t ws_bytes, float* state, void* stream);

/* umpr_adam_step / umpr_adam_step_dev with the gradient scale multiplied by state[COEF] (one float product of the two scalars:
 * with COEF == 1 the update is bit-identical to the unclipped entry points).  state[FINITE] == 0 leaves p, m and v untouched. */
int umpr_adam_step_clip(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                        double eps, double weight_decay, long step, double grad_scale, const float* state, void* stream);
int umpr_adam_step_dev_clip(float* p, const float* g, float* m, float* v, long n, double beta1, double beta2, double eps,
                            const float* hyper, const float* state, void* stream);

/* ---- Per-segment learning-rate and decay multipliers, coupled L2 or AdamW's decoupled decay, in ONE launch ----------------
 * The four forms above behind one entry point: hyper == NULL takes the scalars from lr .. grad_scale as umpr_adam_step does,
 * otherwise from hyper[4] in device memory (lr, weight_decay, step and grad_scale are then ignored); clip_state NULL or the state
 * of umpr_grad_norm as in the _clip forms.  seg_end / seg_lr_mult / seg_wd_mult are HOST arrays of n_segs (1..16) entries, copied
 * into the kernel's arguments: elements [seg_end[k-1], seg_end[k]) of the launch (seg_end[-1] = 0) are updated with the step size
 * step_size * seg_lr_mult[k] and
 *   decoupled == 0: the coupled L2 weight_decay * seg_wd_mult[k] - one float product each, so that multipliers of exactly 1 give
 *     the bits of the plain forms;
 *   decoupled != 0: torch.optim.AdamW - p *= 1 - d first, d = (lr * weight_decay) * (seg_lr_mult[k] * seg_wd_mult[k]), then Adam
 *     on grad_scale * g alone.  hyper[3] then holds lr * weight_decay (in fp32) in place of weight_decay.
 * The ends ascend strictly, every one but the last is a multiple of 64 elements and the last equals n; multipliers are finite,
 * seg_lr_mult > 0, seg_wd_mult >= 0.  Anything else is refused, with a message, before anything is launched.  n == 0 is a
 * successful no-op.  A step that clip_state marks non-finite touches nothing, the decoupled shrink included.  No allocation, no
 * copy, no host synchronisation: capture-safe. */
int umpr_adam_step_groups(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                          double eps, double weight_decay, long step, double grad_scale, const float* hyper /*or NULL*/,
                          const float* clip_state /*or NULL*/, const long* seg_end, const float* seg_lr_mult,
                          const float* seg_wd_mult, int n_segs, int decoupled, void* stream);

/* ---- Gradient accumulation: one optimiser step over several micro-batches ((loss / k).backward() k times, then step()) ----
 * first != 0: acc[i][:] = grads[i][:] - acc is not read, so it needs no zeroing, whatever it holds (the inf or NaN of a skipped
 * step included).  first == 0: acc[i][:] += grads[i][:], one IEEE fp32 add per element, so the chained sum over the micro-batches
 * is the same bits on every run.  The factor 1 / k is not applied here: it goes into the grad_scale of umpr_grad_norm and of the
 * Adam entry points, which then read acc in place of the gradient.  acc / grads / counts are HOST arrays of n_arenas (<= 8)
 * device pointers / element counts, read during the call; any float-aligned pointers and any count >= 0 are accepted (16-byte
 * accesses where acc[i] and grads[i] sit alike inside a 16-byte line, element by element where they do not); acc[i] and grads[i]
 * must not overlap.  n_arenas == 0 or all counts 0 launches nothing.  One launch on a fixed grid; no allocation, no copy, no host
 * synchronisation: capture-safe. */
int umpr_grad_accumulate(float* const* acc, const float* const* grads, const long* counts, int n_arenas, int first, void* stream);

/* ---- Exponential moving average of the parameters (torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(decay)) ----
 * umpr_ema_update, first != 0: ema[i][:] = params[i][:] - ema is not read, so it needs no initialising pass, whatever it holds.
 * first == 0: ema = fmaf(w, params - ema, ema) per element with w = (float)(1 - decay): the difference rounded to float, then one
 * fused multiply-add - the bits of torch.lerp(ema, params, 1 - decay) on the CPU.  decay lies in the open interval (0.5, 1).
 * umpr_arena_swap exchanges a[i][:] and b[i][:] bit for bit (NaN payloads, signed zeros, infinities); a[i] and b[i] must not
 * overlap.  Tables, pointers, counts, alignment and the launch as for umpr_grad_accumulate: HOST arrays of n_arenas (<= 8) device
 * pointers / element counts, any float-aligned pointers, any count >= 0, n_arenas == 0 or all counts 0 launches nothing; everything
 * refused is refused before anything is written.  One launch each on a fixed grid; no allocation, no copy, no host
 * synchronisation. */
int umpr_ema_update(float* const* ema, const float* const* params, const long* counts, int n_arenas, double decay, int first,
                    void* stream);
int umpr_arena_swap(float* const* a, float* const* b, const long* counts, int n_arenas, void* stream);

/* ---- evaluate_mse (src/evaluate.py:12-13, `mse_loss(pred, labels, reduction='sum')` accumulated over batches) -----
 * acc[0] += sum_i (pred[i] - label[i])^2, acc[1] += n; acc = two device doubles the caller zeroed once and reads back
 * once after the last batch (the reference's `.item()` per batch is a host sync per batch). */
int umpr_sq_err_accumulate(const float* pred, const float* label, long n, double* acc, void* stream);

/* ---- test aid: fills the LDS of every CU with NaN (LDS is not cleared between kernels, so a kernel that reads LDS
 * it never wrote shows up as NaN in the parity tests instead of passing by luck).  sink: one int of device memory. */
int umpr_debug_poison_lds(void* sink, void* stream);

/* ---- kernel timing for bench.py's roofline line: while enabled, the library brackets every launch of a kernel
 * family with HIP events on the launch stream.  family: 0 conv3x3 forward (direct implicit GEMM / Winograd),
 * 1 conv3x3 wgrad, 2 generic GEMM, 3 GRU, 4 the Winograd batched GEMM alone (nested inside families 0 and 5; its
 * work is the MFMA FLOPs executed, 1/2.25 of the direct-convolution FLOPs counted for the same launch), 5 the
 * family-0 kernels run as data gradient (these overlap with wgrad on the library's side stream), 6 the Winograd
 * weight-gradient GEMM alone (nested inside family 1, executed FLOPs), 3 the recurrent GRU kernels (work = bytes),
 * 7 / 8 / 9 the bf16 convolution forward / data-gradient / weight-gradient kernels (FLOPs over the padded pixel grid).  read() synchronises the recorded events and returns totals since reset():
 * milliseconds, algorithmic FLOPs, launches. */
int umpr_profile_enable(int on);
int umpr_profile_reset(void);
int umpr_profile_read(int family, double* total_ms, double* total_work, long* launches);

#ifdef __cplusplus
}
#endif
#endif
