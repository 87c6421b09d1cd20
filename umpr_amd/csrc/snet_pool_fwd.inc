// The S-Net pooling forward of text_ops.hip, compiled twice by it (as coattn_fwd_kernels.inc): SNET_MASKED 0 gives
// snet_pool_fwd_kernel<NL>, token for token the kernel from before the padding mask existed; SNET_MASKED 1 gives
// snet_pool_fwd_masked_kernel<NL> with valid [B][S][L] bytes: the softmax runs over the valid tokens of the sentence, P = +0.0 at the
// others, and a sentence without any valid token gets P = 0 and self_atte = 0 (its maximum is -inf and its sum 0: neither enters an
// expf or a division).
//
// one wave per sentence (B*S waves over the grid); the per-sample sum over sentences is snet_senti_kernel
// NL = ceil(L / 64): lane l % 64 holds position l in slot l / 64 (L <= 64 * NL; the reference's max_sent_length is 20, but
// review_level='review' makes whole reviews the "sentences", src/dataset.py:24 - supported up to 256 tokens)
template <int NL>
#if SNET_MASKED
__global__ __launch_bounds__(256) void snet_pool_fwd_masked_kernel(SnetFwdParams p, long nsent, const uint8_t* valid) {
#else
__global__ __launch_bounds__(256) void snet_pool_fwd_kernel(SnetFwdParams p, long nsent) {
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long sent = (long)blockIdx.x * 4 + wave;
  if (sent >= nsent) return;
  const float w = p.Ws[lane];
  const float* X = p.X + sent * p.L * D;
  const float* U = p.U + sent * p.L * AT;
  float e[NL];  // lane l % 64 holds e[l / 64]
#pragma unroll
  for (int k = 0; k < NL; ++k) e[k] = -INFINITY;
  int l = 0;
  for (; l + 3 < p.L; l += 4) {   // four independent reductions in flight (l .. l+3 share a slot: 64 is a multiple of 4)
    const float v0 = wave_sum(w * U[l * AT + lane]);
    const float v1 = wave_sum(w * U[(l + 1) * AT + lane]);
    const float v2 = wave_sum(w * U[(l + 2) * AT + lane]);
    const float v3 = wave_sum(w * U[(l + 3) * AT + lane]);
    const int ll = l & 63;
#pragma unroll
    for (int k = 0; k < NL; ++k)
      if (k == (l >> 6)) e[k] = lane == ll ? v0 : lane == ll + 1 ? v1 : lane == ll + 2 ? v2 : lane == ll + 3 ? v3 : e[k];
  }
  for (; l < p.L; ++l) {
    const float v = wave_sum(w * U[l * AT + lane]);
#pragma unroll
    for (int k = 0; k < NL; ++k)
      if (k == (l >> 6) && lane == (l & 63)) e[k] = v;
  }
#if SNET_MASKED
  bool ok[NL];   // this lane's position of slot k is inside L and valid
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    ok[k] = 64 * k + lane < p.L && valid[sent * p.L + 64 * k + lane] != 0;
    if (!ok[k]) e[k] = -INFINITY;
  }
#endif
  float mx = e[0];
#pragma unroll
  for (int k = 1; k < NL; ++k) mx = fmaxf(mx, e[k]);
  const float m = wave_max(mx);
  float ex[NL], zs = 0.f;
#pragma unroll
#if SNET_MASKED
  for (int k = 0; k < NL; ++k) { ex[k] = ok[k] ? expf(e[k] - m) : 0.f; zs += ex[k]; }
#else
  for (int k = 0; k < NL; ++k) { ex[k] = 64 * k + lane < p.L ? expf(e[k] - m) : 0.f; zs += ex[k]; }
#endif
  const float z = wave_sum(zs);
  float pr[NL];
#pragma unroll
  for (int k = 0; k < NL; ++k) {
#if SNET_MASKED
    pr[k] = ok[k] ? ex[k] / z : 0.f;
#else
    pr[k] = ex[k] / z;
#endif
    if (64 * k + lane < p.L) p.P[sent * p.L + 64 * k + lane] = pr[k];
  }
  float a0 = 0.f, a1 = 0.f;
  for (l = 0; l < p.L; ++l) {
    float src = pr[0];
#pragma unroll
    for (int k = 1; k < NL; ++k) src = (l >> 6) == k ? pr[k] : src;
    const float pl = __shfl(src, l & 63, 64);
    a0 += pl * X[l * D + lane];
    a1 += pl * X[l * D + 64 + lane];
  }
  p.self_atte[sent * D + lane] = a0;
  p.self_atte[sent * D + 64 + lane] = a1;
  float ws = 0.f;
  for (int i = lane; i < p.wl; i += 64) ws += p.word_soft[sent * p.wl + i];
  ws = wave_sum(ws);
  if (lane == 0) p.wsum[sent] = ws;
}
