// The text path of UMPR.forward as TWO calls per direction instead of ~25: the whole ReviewNet (R-Net GRU over the user+item
// review pair, co-attention, the two S-Nets, textual matching - src/model.py:157-169) and the whole ControlNet (C-Net GRU over the
// ui reviews and over the pair, three C-Net heads, control S-Net, SS-Net gate - src/model.py:179-198).  Round 3: a training step
// of UMPR-R is 0.9 ms of kernels, and a host that issues every stage through Python (one ctypes call, a handful of tensor
// allocations and an autograd node each) needs longer than that to enqueue them; here the stages are issued back to back from
// C++ into ONE caller-owned arena (everything the backward pass reads) and one scratch buffer.  The stage functions are the
// internal forms of the per-stage entry points of api.hip: these wrappers only carve buffers and call them in order, each with the
// call's one GEMM precision (gemm_b16: the entry point's b16_gemm argument or the thread's umpr_set_gemm_bf16).
#include <algorithm>

#include "umpr_common.h"
#include "umpr_internal.h"
#include "../../include/umpr_hip.h"

namespace {

constexpr size_t kAlign = 256;   // every piece of an arena or of a workspace prefix starts on a 256-byte boundary

struct SnetSaved { float *U, *P, *wsum, *sa; };
SnetSaved take_snet(Carve& c, long B, long S, long L) {
  SnetSaved s;
  s.U = c.take<float>(B * S * L * AT); s.P = c.take<float>(B * S * L); s.wsum = c.take<float>(B * S); s.sa = c.take<float>(B * S * D);
  return s;
}

// ---- ReviewNet arena ----------------------------------------------------------------------------------------------
struct ReviewArena {
  float *gru_out, *gru_saved, *T, *soft_u, *soft_i, *colmax, *rowmax, *repr_u, *repr_i, *merged;
  int32_t *argcol, *argrow;
  SnetSaved su, si;
  size_t bytes;
};
ReviewArena review_arena(void* base, long B, long S, long L) {
  Carve c(base, kAlign);
  const long N = B * S, SL = S * L;
  ReviewArena a;
  a.gru_out = c.take<float>(2 * N * L * D);
  a.gru_saved = c.take<float>(2 * 2 * N * L * 4 * H);
  a.T = c.take<float>(B * SL * D);
  a.soft_u = c.take<float>(B * SL); a.soft_i = c.take<float>(B * SL);
  a.colmax = c.take<float>(B * SL); a.rowmax = c.take<float>(B * SL);
  a.argcol = c.take<int32_t>(B * SL); a.argrow = c.take<int32_t>(B * SL);
  a.repr_u = c.take<float>(B * 2 * D); a.repr_i = c.take<float>(B * 2 * D);
  a.merged = c.take<float>(B * D);
  a.su = take_snet(c, B, S, L); a.si = take_snet(c, B, S, L);
  a.bytes = c.off;
  return a;
}

// ---- ControlNet arena ---------------------------------------------------------------------------------------------
struct HeadSaved { float *cmax, *sp, *vp, *fin; int32_t* argl; };
struct ControlArena {
  float *gru_ui, *saved_ui, *gru_pair, *saved_pair, *senti, *vs;
  HeadSaved h[3];   // ui, user, item
  SnetSaved sn;
  size_t bytes;
};
ControlArena control_arena(void* base, long B, long S_ui, long L_ui, long S, long L, long KC, long V) {
  Carve c(base, kAlign);
  const long Nui = B * S_ui, N = B * S;
  ControlArena a;
  a.gru_ui = c.take<float>(Nui * L_ui * D);
  a.saved_ui = c.take<float>(2 * Nui * L_ui * 4 * H);
  a.gru_pair = c.take<float>(2 * N * L * D);
  a.saved_pair = c.take<float>(2 * 2 * N * L * 4 * H);
  const long ss[3] = {S_ui, S, S};
  for (int q = 0; q < 3; ++q) {
    a.h[q].cmax = c.take<float>(B * ss[q] * KC); a.h[q].argl = c.take<int32_t>(B * ss[q] * KC);
    a.h[q].sp = c.take<float>(B * ss[q] * V); a.h[q].vp = c.take<float>(B * ss[q] * V); a.h[q].fin = c.take<float>(B * V);
  }
  a.sn = take_snet(c, B, S_ui, L_ui);
  a.senti = c.take<float>(B * S_ui); a.vs = c.take<float>(B * V);
  a.bytes = c.off;
  return a;
}

// ---- workspaces: [the buffers that live across stages][the stage workspace: the largest any stage asks for, + 256] ------
// umpr_review_net_bwd (the forward hands the whole buffer to its stages); dG is also the GRUs' dout
struct ReviewWs { float *dG, *d_repr_u, *d_repr_i, *ds_u, *ds_i, *stage; size_t prefix, bytes; };
ReviewWs review_ws(void* base, int B, int S, int L, int E) {
  Carve c(base, kAlign);
  const long N = (long)B * S, SL = (long)S * L;
  ReviewWs w;
  w.dG = c.take<float>(2 * N * L * D);
  w.d_repr_u = c.take<float>(B * 2 * D); w.d_repr_i = c.take<float>(B * 2 * D);
  w.ds_u = c.take<float>(B * SL); w.ds_i = c.take<float>(B * SL);
  w.stage = c.at<float>(c.off); w.prefix = c.off;
  w.bytes = c.off + 256 + std::max({umpr_embed_gru_bidir_ws_bytes((int)(2 * N), L, E), umpr_coattention_fwd_ws_bytes(B, (int)SL),
                                    umpr_coattention_bwd_ws_bytes(B, (int)SL), umpr_snet_bwd_ws_bytes(B, S, L),
                                    umpr_review_merge_bwd_ws_bytes(B)});
  return w;
}
struct ControlWs {
  float *dX_ui, *dX_pair, *d_sa, *d_vp, *d_cout;   // dX_*: the two GRUs' dout
  float* zero_senti;   // zero d_senti of the control S-Net (its sentiment output is unused, model.py:185)
  float* Y;            // forward scratch: Y of a C-Net head, then - on purpose - the control S-Net's unused sentiment output
  float* stage; size_t prefix, bytes;
};
ControlWs control_ws(void* base, int B, int S_ui, int L_ui, int S, int L, int E, int KC, int KS, int V) {
  Carve c(base, kAlign);
  const long Nui = (long)B * S_ui, N = (long)B * S;
  ControlWs w;
  w.dX_ui = c.take<float>(Nui * L_ui * D); w.dX_pair = c.take<float>(2 * N * L * D);
  w.d_sa = c.take<float>(B * S_ui * D); w.d_vp = c.take<float>(B * S_ui * V); w.d_cout = c.take<float>(B * V);
  w.zero_senti = c.take<float>(B * D);
  w.Y = c.take<float>((long)B * (S_ui > S ? S_ui : S) * (L_ui > L ? L_ui : L) * KC);
  w.stage = c.at<float>(c.off); w.prefix = c.off;
  w.bytes = c.off + 256 + std::max({umpr_embed_gru_bidir_ws_bytes((int)(2 * N), L, E), umpr_embed_gru_bidir_ws_bytes((int)Nui, L_ui, E),
                                    umpr_cnet_head_fwd_ws_bytes(B, S_ui, L_ui, KS), umpr_cnet_head_fwd_ws_bytes(B, S, L, KS),
                                    umpr_cnet_head_bwd_ws_bytes(B, S_ui, L_ui, KC, KS, V), umpr_cnet_head_bwd_ws_bytes(B, S, L, KC, KS, V),
                                    umpr_snet_bwd_ws_bytes(B, S_ui, L_ui), umpr_control_gate_bwd_ws_bytes(B)});
  return w;
}

// UMPR_POISON_WS=1 (debugging aid): every entry point below first fills its workspace - and the forward ones their arena - with
// 0xFF bytes (NaN as floats), so that any read of memory the call did not write itself shows up as NaN in its results instead of
// depending on what the allocator handed out (tests/test_gpu_parity.py::test_text_path_reads_no_uninitialised_memory).
// UMPR_DEBUG_SYNC=<bit mask> (debugging aid): device-wide synchronisation at numbered points of umpr_review_net_bwd (bit 0: on
// entry, 1: after the merge, 2 / 3: after the user / item S-Net, 4: after the co-attention) - narrows a cross-stream dependency down
void debug_sync(int point) {
  static const int mask = umpr_env_int("UMPR_DEBUG_SYNC", 0);
  if (mask & (1 << point)) (void)hipDeviceSynchronize();
}
int poison(void* p, size_t bytes, void* stream) {
  static const bool on = umpr_env_int("UMPR_POISON_WS", 0) == 1;
  if (!on || !p || !bytes) return 0;
  if (hipMemsetAsync(p, 0xFF, bytes, static_cast<hipStream_t>(stream)) != hipSuccess) { umpr_set_error("poison: memset failed"); return -2; }
  return 0;
}

}  // namespace

extern "C" {

// ids of the user and of the item reviews as ONE [2N][L] tensor for the GRUs the two share (src/model.py:45-46, 183-184)
int umpr_concat_ids(const int64_t* ids_u, const int64_t* ids_i, long n_each, int64_t* dst, void* stream) {
  UMPR_REQUIRE(ids_u && ids_i && dst && n_each > 0, "concat_ids: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemcpyAsync(dst, ids_u, (size_t)n_each * 8, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(dst + n_each, ids_i, (size_t)n_each * 8, hipMemcpyDeviceToDevice, s) != hipSuccess) {
    umpr_set_error("concat_ids: copy failed");
    return -2;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------ ReviewNet
size_t umpr_review_net_arena_bytes(int B, int S, int L) { return review_arena(nullptr, B, S, L).bytes; }
size_t umpr_review_net_ws_bytes(int B, int S, int L, int E) { return review_ws(nullptr, B, S, L, E).bytes; }

// params: w_ih_f, w_hh_f, b_ih_f, b_hh_f, w_ih_r, w_hh_r, b_ih_r, b_hh_r, M, Ms_u, Ws_u, Ms_i, Ws_i, W_u, W_i
// valid_pair (or null): the validity bytes [2N][L] of umpr_token_mask on ids_pair - user rows [B][S*L], then item rows
// dst_row: the output row of each input row of the pair (umpr_embed_gru_bidir_fwd): `order` for the reference's double un-sort
static int review_net_fwd(const int64_t* ids_pair, const float* emb, int E, const float* const* P, const int32_t* lengths,
                          const int32_t* order, const int32_t* dst_row, int B, int S, int L, bool gemm_b16, int b16_scores,
                          int need_grad, void* arena, float* out, float* ws, size_t ws_bytes, void* stream, const uint8_t* valid_pair) {
  UMPR_REQUIRE(ids_pair && emb && P && lengths && order && dst_row && arena && out && B > 0 && S > 0 && L > 0, "review_net_fwd: bad arguments");
  UMPR_REQUIRE(ws_bytes >= umpr_review_net_ws_bytes(B, S, L, E), "review_net_fwd: workspace too small");
  if (poison(ws, ws_bytes, stream) || poison(arena, umpr_review_net_arena_bytes(B, S, L), stream)) return -2;
  const ReviewArena A = review_arena(arena, B, S, L);
  const int N = B * S, SL = S * L;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = umpr_embed_gru_fwd_impl(ids_pair, emb, E, P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7], lengths, order, dst_row,
                                       2 * N, L, A.gru_out, need_grad ? A.gru_saved : nullptr, ws, ws_bytes, gemm_b16, s)) return rc;
  const float* gru_u = A.gru_out;
  const float* gru_i = A.gru_out + (size_t)N * L * D;
  // the validity bytes of the user and of the item rows, or no mask at all
  const uint8_t* valid_u = valid_pair;
  const uint8_t* valid_i = valid_pair ? valid_pair + (size_t)N * L : nullptr;
  if (int rc = umpr_coattn_fwd_impl(gru_u, gru_i, P[8], B, SL, A.T, A.soft_u, A.soft_i, A.repr_u, 2 * D, A.repr_i, 2 * D, A.colmax,
                                    A.argcol, A.rowmax, A.argrow, ws, ws_bytes, gemm_b16, b16_scores ? 1 : 0, s, valid_u, valid_i))
    return rc;
  if (int rc = umpr_snet_fwd_impl(gru_u, P[9], P[10], A.soft_u, L, B, S, L, A.su.U, A.su.P, A.su.wsum, A.su.sa, A.repr_u + D, 2 * D,
                                  gemm_b16, s, valid_u)) return rc;
  if (int rc = umpr_snet_fwd_impl(gru_i, P[11], P[12], A.soft_i, L, B, S, L, A.si.U, A.si.P, A.si.wsum, A.si.sa, A.repr_i + D, 2 * D,
                                  gemm_b16, s, valid_i)) return rc;
  if (B <= 256 && umpr_merge_small())   // one kernel writes the caller's tensor and the arena's copy for backward
    return umpr_review_merge_fwd_impl(A.repr_u, A.repr_i, P[13], P[14], B, out, A.merged, s);
  if (int rc = umpr_review_merge_fwd_any(A.repr_u, A.repr_i, P[13], P[14], B, A.merged, gemm_b16, s)) return rc;
  if (hipMemcpyAsync(out, A.merged, (size_t)B * D * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    umpr_set_error("review_net_fwd: copy failed");
    return -2;
  }
  return 0;
}

int umpr_review_net_fwd(const int64_t* ids_pair, const float* emb, int E, const float* const* P, const int32_t* lengths,
                        const int32_t* order, int B, int S, int L, int b16_gemm, int b16_scores, int need_grad, void* arena,
                        float* out, float* ws, size_t ws_bytes, void* stream) {
  return review_net_fwd(ids_pair, emb, E, P, lengths, order, order, B, S, L, b16_gemm || umpr_ambient_gemm_b16(), b16_scores, need_grad, arena,
                        out, ws, ws_bytes, stream, nullptr);
}
int umpr_review_net_fwd_masked(const int64_t* ids_pair, const float* emb, int E, const float* const* P, const int32_t* lengths,
                               const int32_t* order, int B, int S, int L, int b16_gemm, int b16_scores, int need_grad,
                               void* arena, float* out, float* ws, size_t ws_bytes, const uint8_t* valid_pair, void* stream) {
  UMPR_REQUIRE(valid_pair, "review_net_fwd_masked: null validity mask");
  return review_net_fwd(ids_pair, emb, E, P, lengths, order, order, B, S, L, b16_gemm || umpr_ambient_gemm_b16(), b16_scores, need_grad, arena,
                        out, ws, ws_bytes, stream, valid_pair);
}
int umpr_review_net_fwd_ex(const int64_t* ids_pair, const float* emb, int E, const float* const* P, const int32_t* lengths,
                           const int32_t* order, const int32_t* dst_row, int B, int S, int L, int b16_gemm, int b16_scores,
                           int need_grad, void* arena, float* out, float* ws, size_t ws_bytes, const uint8_t* valid_pair,
                           void* stream) {
  return review_net_fwd(ids_pair, emb, E, P, lengths, order, dst_row, B, S, L, b16_gemm || umpr_ambient_gemm_b16(), b16_scores, need_grad, arena,
                        out, ws, ws_bytes, stream, valid_pair);
}

// grads: 15 pointers in the order of params, each overwritten; dx_pair (or NULL): the token gradient for a trainable table
static int review_net_bwd(const int64_t* ids_pair, const float* emb, int E, const float* const* P, const int32_t* lengths,
                          const int32_t* order, const int32_t* dst_row, int B, int S, int L, bool gemm_b16, const void* arena,
                          const float* d_out, float* const* G, float* dx_pair, float* ws, size_t ws_bytes, void* stream) {
  UMPR_REQUIRE(ids_pair && emb && P && G && lengths && order && dst_row && arena && d_out, "review_net_bwd: bad arguments");
  const ReviewWs W = review_ws(ws, B, S, L, E);
  UMPR_REQUIRE(ws_bytes >= W.bytes, "review_net_bwd: workspace too small");
  if (poison(ws, ws_bytes, stream)) return -2;
  const ReviewArena A = review_arena(const_cast<void*>(arena), B, S, L);
  const long N = (long)B * S, SL = (long)S * L;
  float *dG = W.dG, *d_repr_u = W.d_repr_u, *d_repr_i = W.d_repr_i, *ds_u = W.ds_u, *ds_i = W.ds_i;
  float* sws = W.stage; const size_t swsb = ws_bytes - W.prefix;
  const float* gru_u = A.gru_out;
  const float* gru_i = A.gru_out + (size_t)N * L * D;
  float* dGu = dG;
  float* dGi = dG + (size_t)N * L * D;
  hipStream_t s = static_cast<hipStream_t>(stream);
  debug_sync(0);
  if (int rc = umpr_review_merge_bwd_any(A.repr_u, A.repr_i, P[13], P[14], A.merged, d_out, B, d_repr_u, d_repr_i, G[13], G[14], sws, swsb,
                                         gemm_b16, s)) return rc;
  debug_sync(1);
  if (int rc = umpr_snet_bwd_impl(gru_u, P[9], P[10], A.su.U, A.su.P, A.su.wsum, A.su.sa, d_repr_u + D, 2 * D, nullptr, B, S, L, L, dGu,
                                  G[9], G[10], ds_u, sws, swsb, gemm_b16, s)) return rc;
  debug_sync(2);
  if (int rc = umpr_snet_bwd_impl(gru_i, P[11], P[12], A.si.U, A.si.P, A.si.wsum, A.si.sa, d_repr_i + D, 2 * D, nullptr, B, S, L, L, dGi,
                                  G[11], G[12], ds_i, sws, swsb, gemm_b16, s)) return rc;
  debug_sync(3);
  if (int rc = umpr_coattn_bwd_impl(gru_u, gru_i, P[8], A.T, A.soft_u, A.soft_i, A.colmax, A.argcol, A.rowmax, A.argrow, d_repr_u,
                                    2 * D, d_repr_i, 2 * D, ds_u, ds_i, B, (int)SL, dGu, dGi, G[8], 1, sws, swsb, gemm_b16, s)) return rc;
  debug_sync(4);
  return umpr_embed_gru_bwd_impl(ids_pair, emb, E, P[1], P[5], lengths, order, dst_row, (int)(2 * N), L, dG, A.gru_out, A.gru_saved,
                                 G[0], G[1], G[2], G[3], G[4], G[5], G[6], G[7], 0, P[0], P[4], dx_pair, 0, sws, swsb, gemm_b16, s);
}
int umpr_review_net_bwd_dx(const int64_t* ids_pair, const float* emb, int E, const float* const* P, const int32_t* lengths,
                           const int32_t* order, int B, int S, int L, int b16_gemm, const void* arena, const float* d_out,
                           float* const* G, float* dx_pair, float* ws, size_t ws_bytes, void* stream) {
  return review_net_bwd(ids_pair, emb, E, P, lengths, order, order, B, S, L, b16_gemm || umpr_ambient_gemm_b16(), arena, d_out, G, dx_pair,
                        ws, ws_bytes, stream);
}
int umpr_review_net_bwd_ex(const int64_t* ids_pair, const float* emb, int E, const float* const* P, const int32_t* lengths,
                           const int32_t* order, const int32_t* dst_row, int B, int S, int L, int b16_gemm, const void* arena,
                           const float* d_out, float* const* G, float* dx_pair, float* ws, size_t ws_bytes, void* stream) {
  return review_net_bwd(ids_pair, emb, E, P, lengths, order, dst_row, B, S, L, b16_gemm || umpr_ambient_gemm_b16(), arena, d_out, G, dx_pair,
                        ws, ws_bytes, stream);
}
int umpr_review_net_bwd(const int64_t* ids_pair, const float* emb, int E, const float* const* P, const int32_t* lengths,
                        const int32_t* order, int B, int S, int L, int b16_gemm, const void* arena, const float* d_out,
                        float* const* G, float* ws, size_t ws_bytes, void* stream) {
  return umpr_review_net_bwd_dx(ids_pair, emb, E, P, lengths, order, B, S, L, b16_gemm, arena, d_out, G, nullptr, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------------ ControlNet
size_t umpr_control_net_arena_bytes(int B, int S_ui, int L_ui, int S, int L, int KC, int V) {
  return control_arena(nullptr, B, S_ui, L_ui, S, L, KC, V).bytes;
}
size_t umpr_control_net_ws_bytes(int B, int S_ui, int L_ui, int S, int L, int E, int KC, int KS, int V) {
  return control_ws(nullptr, B, S_ui, L_ui, S, L, E, KC, KS, V).bytes;
}

// params: the C-Net GRU's eight (as above), Wc [KC][128][KS], bc, Wl [V][KC], bl, Ms, Ws, ssW [128], ssb [1]
// dst_ui / dst_pair: the output row of each input row of the two GRU calls (ord_* for the reference's double un-sort);
// valid_ui [B*S_ui][L_ui], valid_pair [2N][L] (both or neither): the validity bytes of umpr_token_mask on ids_ui / ids_pair
static int control_net_fwd(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* P,
                           const int32_t* len_ui, const int32_t* ord_ui, const int32_t* dst_ui, const int32_t* len_pair,
                           const int32_t* ord_pair, const int32_t* dst_pair, int B, int S_ui, int L_ui, int S, int L, int KC, int KS,
                           int V, float thr, bool gemm_b16, int need_grad, void* arena, float* c_u, float* c_i, float* prefer_pos,
                           float* prefer_neg, float* ws, size_t ws_bytes, void* stream, const uint8_t* valid_ui,
                           const uint8_t* valid_pair) {
  UMPR_REQUIRE((valid_ui == nullptr) == (valid_pair == nullptr), "control_net_fwd: valid_ui and valid_pair go together");
  UMPR_REQUIRE(ids_ui && ids_pair && emb && P && arena && c_u && c_i && prefer_pos && prefer_neg && dst_ui && dst_pair,
               "control_net_fwd: bad arguments");
  const ControlWs W = control_ws(ws, B, S_ui, L_ui, S, L, E, KC, KS, V);
  UMPR_REQUIRE(ws_bytes >= W.bytes, "control_net_fwd: workspace too small");
  if (poison(ws, ws_bytes, stream) || poison(arena, umpr_control_net_arena_bytes(B, S_ui, L_ui, S, L, KC, V), stream)) return -2;
  const ControlArena A = control_arena(arena, B, S_ui, L_ui, S, L, KC, V);
  const long Nui = (long)B * S_ui, N = (long)B * S;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = umpr_embed_gru_fwd_impl(ids_ui, emb, E, P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7], len_ui, ord_ui, dst_ui, (int)Nui,
                                       L_ui, A.gru_ui, need_grad ? A.saved_ui : nullptr, ws, ws_bytes, gemm_b16, s)) return rc;
  if (int rc = umpr_embed_gru_fwd_impl(ids_pair, emb, E, P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7], len_pair, ord_pair, dst_pair,
                                       (int)(2 * N), L, A.gru_pair, need_grad ? A.saved_pair : nullptr, ws, ws_bytes, gemm_b16, s)) return rc;
  float* Y = W.Y;   // (the GRUs above used the whole buffer)
  float* sws = W.stage; const size_t swsb = ws_bytes - W.prefix;
  const float* X[3] = {A.gru_ui, A.gru_pair, A.gru_pair + (size_t)N * L * D};
  const int ss[3] = {S_ui, S, S}, ll[3] = {L_ui, L, L};
  // the validity bytes of the three heads' rows, or no mask at all
  const uint8_t* vv[3] = {valid_ui, valid_pair, valid_pair ? valid_pair + (size_t)N * L : nullptr};
  for (int q = 0; q < 3; ++q)
    if (int rc = umpr_cnet_head_fwd_impl(X[q], P[8], P[9], P[10], P[11], thr, B, ss[q], ll[q], KC, KS, V, Y, A.h[q].cmax, A.h[q].argl,
                                         A.h[q].sp, A.h[q].vp, A.h[q].fin, sws, swsb, gemm_b16, s, vv[q])) return rc;
  // control S-Net weighted by view_p (model.py:185); its sentiment vector is not used: written into scratch
  if (int rc = umpr_snet_fwd_impl(A.gru_ui, P[12], P[13], A.h[0].vp, V, B, S_ui, L_ui, A.sn.U, A.sn.P, A.sn.wsum, A.sn.sa, Y, D,
                                  gemm_b16, s, valid_ui)) return rc;
  if (int rc = umpr_gate_fwd_impl(A.sn.sa, P[14], P[15], A.h[0].vp, A.h[0].fin, B, S_ui, V, A.senti, A.vs, prefer_pos, prefer_neg, s)) return rc;
  if (hipMemcpyAsync(c_u, A.h[1].fin, (size_t)B * V * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(c_i, A.h[2].fin, (size_t)B * V * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    umpr_set_error("control_net_fwd: copy failed");
    return -2;
  }
  return 0;
}
int umpr_control_net_fwd(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* P,
                         const int32_t* len_ui, const int32_t* ord_ui, const int32_t* len_pair, const int32_t* ord_pair, int B,
                         int S_ui, int L_ui, int S, int L, int KC, int KS, int V, float thr, int b16_gemm, int need_grad, void* arena,
                         float* c_u, float* c_i, float* prefer_pos, float* prefer_neg, float* ws, size_t ws_bytes, void* stream) {
  return control_net_fwd(ids_ui, ids_pair, emb, E, P, len_ui, ord_ui, ord_ui, len_pair, ord_pair, ord_pair, B, S_ui, L_ui, S, L, KC, KS,
                         V, thr, b16_gemm || umpr_ambient_gemm_b16(), need_grad, arena, c_u, c_i, prefer_pos, prefer_neg, ws, ws_bytes,
                         stream, nullptr, nullptr);
}
int umpr_control_net_fwd_ex(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* P,
                            const int32_t* len_ui, const int32_t* ord_ui, const int32_t* dst_ui, const int32_t* len_pair,
                            const int32_t* ord_pair, const int32_t* dst_pair, int B, int S_ui, int L_ui, int S, int L, int KC, int KS,
                            int V, float thr, int b16_gemm, int need_grad, void* arena, float* c_u, float* c_i, float* prefer_pos,
                            float* prefer_neg, float* ws, size_t ws_bytes, const uint8_t* valid_ui, const uint8_t* valid_pair,
                            void* stream) {
  return control_net_fwd(ids_ui, ids_pair, emb, E, P, len_ui, ord_ui, dst_ui, len_pair, ord_pair, dst_pair, B, S_ui, L_ui, S, L, KC, KS,
                         V, thr, b16_gemm || umpr_ambient_gemm_b16(), need_grad, arena, c_u, c_i, prefer_pos, prefer_neg, ws, ws_bytes,
                         stream, valid_ui, valid_pair);
}

// d_cu, d_ci, d_pp, d_pn [B][V]; grads: 16 pointers in the order of params, each overwritten
// dx_pair / dx_ui (both or neither): the token gradients of the C-Net GRU's two calls for a trainable table
static int control_net_bwd(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* P,
                           const int32_t* len_ui, const int32_t* ord_ui, const int32_t* dst_ui, const int32_t* len_pair,
                           const int32_t* ord_pair, const int32_t* dst_pair, int B, int S_ui, int L_ui, int S, int L, int KC, int KS,
                           int V, bool gemm_b16, const void* arena, const float* d_cu, const float* d_ci, const float* d_pp,
                           const float* d_pn, float* const* G, float* dx_pair, float* dx_ui, float* ws, size_t ws_bytes, void* stream) {
  UMPR_REQUIRE((dx_pair == nullptr) == (dx_ui == nullptr), "control_net_bwd: dx_pair and dx_ui go together");
  UMPR_REQUIRE(ids_ui && ids_pair && emb && P && G && arena && d_cu && d_ci && d_pp && d_pn && dst_ui && dst_pair,
               "control_net_bwd: bad arguments");
  const ControlWs W = control_ws(ws, B, S_ui, L_ui, S, L, E, KC, KS, V);
  UMPR_REQUIRE(ws_bytes >= W.bytes, "control_net_bwd: workspace too small");
  if (poison(ws, ws_bytes, stream)) return -2;
  const ControlArena A = control_arena(const_cast<void*>(arena), B, S_ui, L_ui, S, L, KC, V);
  const long Nui = (long)B * S_ui, N = (long)B * S;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float *dX_ui = W.dX_ui, *dX_pair = W.dX_pair, *d_sa = W.d_sa, *d_vp = W.d_vp, *d_cout = W.d_cout, *zero_senti = W.zero_senti;
  float* sws = W.stage; const size_t swsb = ws_bytes - W.prefix;
  if (hipMemsetAsync(zero_senti, 0, (size_t)B * D * sizeof(float), s) != hipSuccess) { umpr_set_error("control_net_bwd: memset"); return -2; }
  if (int rc = umpr_gate_bwd_impl(A.sn.sa, P[14], A.h[0].vp, A.h[0].fin, A.senti, A.vs, d_pp, d_pn, B, S_ui, V, d_sa, d_vp, d_cout,
                                  G[14], G[15], sws, swsb, s)) return rc;
  if (int rc = umpr_snet_bwd_impl(A.gru_ui, P[12], P[13], A.sn.U, A.sn.P, A.sn.wsum, A.sn.sa, zero_senti, D, d_sa, B, S_ui, L_ui, V, dX_ui,
                                  G[12], G[13], nullptr, sws, swsb, gemm_b16, s)) return rc;
  const float* X[3] = {A.gru_ui, A.gru_pair, A.gru_pair + (size_t)N * L * D};
  float* dX[3] = {dX_ui, dX_pair, dX_pair + (size_t)N * L * D};
  const float* dfin[3] = {d_cout, d_cu, d_ci};
  const float* dvp[3] = {d_vp, nullptr, nullptr};
  const int ss[3] = {S_ui, S, S}, ll[3] = {L_ui, L, L};
  for (int q = 0; q < 3; ++q)   // the ui head adds onto the S-Net's dX and writes the weight gradients; the other two add onto those
    if (int rc = umpr_cnet_head_bwd_impl(X[q], P[8], P[10], A.h[q].cmax, A.h[q].argl, A.h[q].sp, A.h[q].vp, dfin[q], dvp[q], B, ss[q], ll[q],
                                         KC, KS, V, dX[q], q == 0 ? 1 : 0, q == 0 ? 0 : 1, G[8], G[9], G[10], G[11], sws, swsb, gemm_b16, s))
      return rc;
  if (int rc = umpr_embed_gru_bwd_impl(ids_ui, emb, E, P[1], P[5], len_ui, ord_ui, dst_ui, (int)Nui, L_ui, dX_ui, A.gru_ui, A.saved_ui,
                                       G[0], G[1], G[2], G[3], G[4], G[5], G[6], G[7], 0, P[0], P[4], dx_ui, 0, sws, swsb, gemm_b16, s)) return rc;
  return umpr_embed_gru_bwd_impl(ids_pair, emb, E, P[1], P[5], len_pair, ord_pair, dst_pair, (int)(2 * N), L, dX_pair, A.gru_pair,
                                 A.saved_pair, G[0], G[1], G[2], G[3], G[4], G[5], G[6], G[7], 1, P[0], P[4], dx_pair, 0, sws, swsb,
                                 gemm_b16, s);
}
int umpr_control_net_bwd_dx(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* P,
                            const int32_t* len_ui, const int32_t* ord_ui, const int32_t* len_pair, const int32_t* ord_pair, int B,
                            int S_ui, int L_ui, int S, int L, int KC, int KS, int V, int b16_gemm, const void* arena, const float* d_cu,
                            const float* d_ci, const float* d_pp, const float* d_pn, float* const* G, float* dx_pair, float* dx_ui,
                            float* ws, size_t ws_bytes, void* stream) {
  return control_net_bwd(ids_ui, ids_pair, emb, E, P, len_ui, ord_ui, ord_ui, len_pair, ord_pair, ord_pair, B, S_ui, L_ui, S, L, KC, KS,
                         V, b16_gemm || umpr_ambient_gemm_b16(), arena, d_cu, d_ci, d_pp, d_pn, G, dx_pair, dx_ui, ws, ws_bytes, stream);
}
int umpr_control_net_bwd_ex(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* P,
                            const int32_t* len_ui, const int32_t* ord_ui, const int32_t* dst_ui, const int32_t* len_pair,
                            const int32_t* ord_pair, const int32_t* dst_pair, int B, int S_ui, int L_ui, int S, int L, int KC, int KS,
                            int V, int b16_gemm, const void* arena, const float* d_cu, const float* d_ci, const float* d_pp,
                            const float* d_pn, float* const* G, float* dx_pair, float* dx_ui, float* ws, size_t ws_bytes,
                            void* stream) {
  return control_net_bwd(ids_ui, ids_pair, emb, E, P, len_ui, ord_ui, dst_ui, len_pair, ord_pair, dst_pair, B, S_ui, L_ui, S, L, KC, KS,
                         V, b16_gemm || umpr_ambient_gemm_b16(), arena, d_cu, d_ci, d_pp, d_pn, G, dx_pair, dx_ui, ws, ws_bytes, stream);
}
int umpr_control_net_bwd(const int64_t* ids_ui, const int64_t* ids_pair, const float* emb, int E, const float* const* P,
                         const int32_t* len_ui, const int32_t* ord_ui, const int32_t* len_pair, const int32_t* ord_pair, int B,
                         int S_ui, int L_ui, int S, int L, int KC, int KS, int V, int b16_gemm, const void* arena, const float* d_cu,
                         const float* d_ci, const float* d_pp, const float* d_pn, float* const* G, float* ws, size_t ws_bytes,
                         void* stream) {
  return umpr_control_net_bwd_dx(ids_ui, ids_pair, emb, E, P, len_ui, ord_ui, len_pair, ord_pair, B, S_ui, L_ui, S, L, KC, KS, V, b16_gemm,
                                 arena, d_cu, d_ci, d_pp, d_pn, G, nullptr, nullptr, ws, ws_bytes, stream);
}

}  // extern "C"
