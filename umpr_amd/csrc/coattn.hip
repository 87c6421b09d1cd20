// R-Net co-attention (src/model.py:50-55) for gfx950, hidden width 2u = 128.
//
//   A = tanh(G_i M G_u^T)   soft_u = softmax_k(max_j A[j,k])   soft_i = softmax_j(max_k A[j,k])
//   atte_u = G_u^T soft_u   atte_i = G_i^T soft_i
//
// The reference has no padding mask, and neither have umpr_coattention_fwd / _fwd_bf16.  umpr_coattention_fwd_masked takes
// one validity byte per user and per item position: maxima run over valid partners only, an undefined position (masked,
// or without any valid partner) is saved as colmax = +0.0, argcol = -1, soft = +0.0, and the softmax runs over the
// defined positions alone (a side without any gets soft = 0 and atte = 0).  The backward needs no mask: soft = 0 makes
// dS = 0 there, and coattn_bwd_rows_kernel forms no address from a negative index.  The forward kernels live in
// coattn_fwd_kernels.inc and are compiled twice from it, without and with the mask: the unmasked ones are the text, and
// compile to the code, they were before the mask existed.
//
// The SLxSL affinity matrix is never written to HBM: T = G_i M comes from the GEMM kernel, `scores` forms 64x64
// tiles of tanh(T G_u^T) on v_mfma_f32_32x32x2_f32 and keeps only row/column maxima with their (first) argmax, and
// the backward is sparse (<= 2*SL non-zeros of dA per sample), routed through the saved argmax indices.
#include "umpr_common.h"
#include "umpr_internal.h"

namespace {


struct ScoreParams {
  const float* T;   // [B][SL][128] = G_i M
  const float* Gu;  // [B][SL][128]
  float* rowmax_part; int* argrow_part;  // [B][ksplit][SL]: maxima over the column tiles of one split
  float* colmax_part; int* argcol_part;  // [B][nblk][SL]
  int SL, nblk, ksplit;                  // grid (nblk row blocks, B, ksplit): column tiles are dealt out over blockIdx.z
};

__device__ __forceinline__ void better_first(float& v, int& i, float v2, int i2) {
  // keep the maximum; on ties the smaller index (first occurrence)
  if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

// 64 rows x 128 columns of src (rows past SL as zeros) -> dst[row][LDR], row-major: float4 in, float4 out.  All eight
// loads of a thread are issued before the first is used, with clamped row addresses: a per-lane `valid ? load : 0`
// makes hipcc wait for each load inside its branch (one global round trip per element, ~15 us per tile).
constexpr int LDR = 132;   // 16 lanes x ds_read_b128 at a row stride of 132 floats touch 64 distinct banks
__device__ __forceinline__ void stage_tile_f32(const float* __restrict__ src, int row0, int SL, float* __restrict__ dst,
                                               int tid) {
  float4 v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = tid + 256 * i;
    const int j = e >> 5, c4 = (e & 31) * 4;
    v[i] = *reinterpret_cast<const float4*>(src + (long)min(row0 + j, SL - 1) * D + c4);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = tid + 256 * i;
    const int j = e >> 5, c4 = (e & 31) * 4;
    *reinterpret_cast<float4*>(dst + j * LDR + c4) = row0 + j < SL ? v[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
__device__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
  return s;
}
__device__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s = fmaxf(s, red[w]);
  return s;
}

struct FinishParams {
  const float* Gu; const float* Gi;
  const float* colmax_part; const int* argcol_part; int nblk;
  const float* rowmax_part; const int* argrow_part; int ksplit;
  float* rowmax; int* argrow;
  float* colmax; int* argcol;
  float* soft_u; float* soft_i;
  float* atte_u; long ld_u;  // atte_u[b*ld_u + c]
  float* atte_i; long ld_i;
  int SL;
};

// coattn_scores_kernel, coattn_scores_bf16_kernel, coattn_finish_kernel and their *_masked_kernel forms
#define COATTN_MASKED 0
#include "coattn_fwd_kernels.inc"
#undef COATTN_MASKED
#define COATTN_MASKED 1
#include "coattn_fwd_kernels.inc"
#undef COATTN_MASKED

struct BwdPrepParams {
  const float* Gu; const float* Gi;
  const float* d_atte_u; long ld_du; const float* d_atte_i; long ld_di;   // [B][128] (strided rows)
  const float* d_soft_u; const float* d_soft_i;                           // [B][SL] or null
  const float* soft_u; const float* soft_i; const float* colmax; const float* rowmax;
  float* dSc; float* dSr;  // [B][SL]
  int SL;
};

// grid (B, 2): one workgroup per (sample, side), as coattn_finish_kernel.  No mask is needed after a masked forward: an undefined
// position has soft = 0 and max = 0, so it adds 0 to dsum and gets dS = 0 (G and d_soft are finite there).
__global__ __launch_bounds__(1024) void coattn_bwd_prep_kernel(BwdPrepParams p) {
  extern __shared__ float sm[];  // ds[SL]
  __shared__ float red[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, side = blockIdx.y, SL = p.SL;
  float* ds = sm;
  const float* Gs = (side ? p.Gi : p.Gu) + (long)b * SL * D;
  const float* d_atte = side ? p.d_atte_i + (long)b * p.ld_di : p.d_atte_u + (long)b * p.ld_du;
  const float* d_soft = side ? p.d_soft_i : p.d_soft_u;
  const float* soft = (side ? p.soft_i : p.soft_u) + (long)b * SL;
  const float* vmax = (side ? p.rowmax : p.colmax) + (long)b * SL;
  float* dS = (side ? p.dSr : p.dSc) + (long)b * SL;
  const float da0 = d_atte[lane], da1 = d_atte[64 + lane];
  for (int k = wave; k < SL; k += 32) {        // two positions per trip: both rows' loads in flight before either reduction
    const int k2 = k + 16;
    const bool has2 = k2 < SL;
    const float* g = Gs + (long)k * D;
    const float* g2 = Gs + (long)(has2 ? k2 : k) * D;
    const float a0 = g[lane], a1 = g[64 + lane], b0 = g2[lane], b1 = g2[64 + lane];
    const float v = wave_sum(a0 * da0 + a1 * da1);
    const float v2 = wave_sum(b0 * da0 + b1 * da1);
    if (lane == 0) {
      ds[k] = v + (d_soft ? d_soft[(long)b * SL + k] : 0.f);
      if (has2) ds[k2] = v2 + (d_soft ? d_soft[(long)b * SL + k2] : 0.f);
    }
  }
  __syncthreads();
  float dsum = 0.f;
  for (int k = tid; k < SL; k += 1024) dsum += soft[k] * ds[k];
  dsum = block_sum(dsum, red);
  for (int k = tid; k < SL; k += 1024) {
    const float m = vmax[k];
    dS[k] = soft[k] * (ds[k] - dsum) * (1.f - m * m);
  }
}

struct BwdRowsParams {
  const float* Gu; const float* T;
  const float* soft_u; const float* soft_i;
  const float* d_atte_u; long ld_du; const float* d_atte_i; long ld_di;
  const float* dSc; const float* dSr; const int* argcol; const int* argrow;
  float* dGu;  // [B][SL][128]  = soft_u d_atte_u + routed dS T
  float* dT;   // [B][SL][128]
  float* dGi;  // [B][SL][128]  initialised with soft_i d_atte_i (the GEMM dT M^T accumulates onto it)
  int SL; int accumulate;  // accumulate: add onto the caller's dGu / dGi instead of overwriting
};

__global__ __launch_bounds__(256) void coattn_bwd_rows_kernel(BwdRowsParams p) {
  extern __shared__ float sm[];  // dSc[SL], dSr[SL], argcol[SL], argrow[SL]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, SL = p.SL;
  float* sc = sm; float* sr = sm + SL;
  int* ac = reinterpret_cast<int*>(sm + 2 * SL); int* ar = ac + SL;
  for (int k = tid; k < SL; k += 256) {
    const long o = (long)b * SL + k;
    sc[k] = p.dSc[o]; sr[k] = p.dSr[o]; ac[k] = p.argcol[o]; ar[k] = p.argrow[o];
  }
  __syncthreads();
  const float* Gu = p.Gu + (long)b * SL * D;
  const float* T = p.T + (long)b * SL * D;
  const float dau0 = p.d_atte_u[(long)b * p.ld_du + lane], dau1 = p.d_atte_u[(long)b * p.ld_du + 64 + lane];
  const float dai0 = p.d_atte_i[(long)b * p.ld_di + lane], dai1 = p.d_atte_i[(long)b * p.ld_di + 64 + lane];
  const int rows_per_block = 16;
  const int r0 = blockIdx.x * rows_per_block;
  for (int rr = wave; rr < rows_per_block; rr += 4) {
    const int row = r0 + rr;
    if (row >= SL) break;
    const long o = ((long)b * SL + row) * D;
    // ---- dG_u[row] (row is a u position k)
    {
      const float su = p.soft_u[(long)b * SL + row];
      const int j = ac[row];
      const float w = sc[row];
      float a0 = 0.f, a1 = 0.f;            // j = -1 (masked forward: an undefined position, soft_u = 0): no address from it
      if (j >= 0) {
        a0 = su * dau0 + w * T[(long)j * D + lane];
        a1 = su * dau1 + w * T[(long)j * D + 64 + lane];
      }
      for (int base = 0; base < SL; base += 64) {
        const int jj = base + lane;
        unsigned long long m = __ballot(jj < SL && ar[jj] == row);
        while (m) {
          const int q = base + __builtin_ctzll(m);
          m &= m - 1;
          const float wq = sr[q];
          a0 += wq * T[(long)q * D + lane];
          a1 += wq * T[(long)q * D + 64 + lane];
        }
      }
      if (p.accumulate) { a0 += p.dGu[o + lane]; a1 += p.dGu[o + 64 + lane]; }
      p.dGu[o + lane] = a0; p.dGu[o + 64 + lane] = a1;
    }
    // ---- dT[row] (row is an i position j)
    {
      const int k = ar[row];
      const float w = sr[row];
      float a0 = 0.f, a1 = 0.f;            // k = -1: as above
      if (k >= 0) {
        a0 = w * Gu[(long)k * D + lane];
        a1 = w * Gu[(long)k * D + 64 + lane];
      }
      for (int base = 0; base < SL; base += 64) {
        const int kk = base + lane;
        unsigned long long m = __ballot(kk < SL && ac[kk] == row);
        while (m) {
          const int q = base + __builtin_ctzll(m);
          m &= m - 1;
          const float wq = sc[q];
          a0 += wq * Gu[(long)q * D + lane];
          a1 += wq * Gu[(long)q * D + 64 + lane];
        }
      }
      p.dT[o + lane] = a0; p.dT[o + 64 + lane] = a1;
      const float si = p.soft_i[(long)b * SL + row];
      float g0 = k >= 0 ? si * dai0 : 0.f, g1 = k >= 0 ? si * dai1 : 0.f;
      if (p.accumulate) { g0 += p.dGi[o + lane]; g1 += p.dGi[o + 64 + lane]; }
      p.dGi[o + lane] = g0; p.dGi[o + 64 + lane] = g1;
    }
  }
}

// forward workspace: per-tile partial maxima of the score matrix and their positions, [B][nblk][SL] each, over the columns
// (cpart | apart) and over the rows (rpart | arpart); nblk = cdiv(SL, 64) score tiles per side
struct CoattnFwdWs { float* cpart; int* apart; float* rpart; int* arpart; size_t bytes; };
CoattnFwdWs coattn_fwd_ws(float* base, int B, int SL) {
  Carve c(base, sizeof(float));
  const size_t n = (size_t)B * cdiv(SL, 64) * SL;
  return CoattnFwdWs{c.take<float>(n), c.take<int>(n), c.take<float>(n), c.take<int>(n), c.off};
}
// backward workspace: dSc | dSr [B*SL] | dT [B*SL][128] | split-K slab of the dM product
struct CoattnBwdWs { float *dSc, *dSr, *dT, *slab; size_t slab_bytes, bytes; };
CoattnBwdWs coattn_bwd_ws(float* base, int B, int SL) {
  Carve c(base, sizeof(float));
  const size_t n = (size_t)B * SL, nslab = (size_t)512 * D * D;
  return CoattnBwdWs{c.take<float>(n), c.take<float>(n), c.take<float>(n * D), c.take<float>(nslab), nslab * sizeof(float), c.off};
}

}  // namespace

size_t umpr_coattn_fwd_ws_bytes(int B, int SL) { return coattn_fwd_ws(nullptr, B, SL).bytes; }

int umpr_coattn_fwd_impl(const float* Gu, const float* Gi, const float* M, int B, int SL, float* T, float* soft_u,
                         float* soft_i, float* atte_u, long ld_u, float* atte_i, long ld_i, float* colmax, int* argcol,
                         float* rowmax, int* argrow, float* ws, size_t ws_bytes, bool gemm_b16, int bf16_scores, hipStream_t s,
                         const uint8_t* valid_u, const uint8_t* valid_i) {
  UMPR_REQUIRE(B > 0 && SL > 0, "coattn: bad shape");
  UMPR_REQUIRE(!valid_u == !valid_i, "coattn: one validity mask without the other");
  const bool masked = valid_u != nullptr;
  const CoattnFwdWs W = coattn_fwd_ws(ws, B, SL);
  UMPR_REQUIRE(ws_bytes >= W.bytes, "coattn: workspace too small");
  const int nblk = cdiv(SL, 64);
  UmprGemm g;
  g.A = Gi; g.lda = D; g.B = M; g.ldb = D; g.C = T; g.ldc = D; g.M = B * SL; g.N = D; g.K = D; g.b16 = gemm_b16;
  if (int rc = umpr_gemm(g, s)) return rc;
  // one 64 x 64 score tile per workgroup: nblk^2 * B workgroups instead of nblk * B serial tile loops
  const int ksplit = nblk;
  ScoreParams sp{T, Gu, W.rpart, W.arpart, W.cpart, W.apart, SL, nblk, ksplit};
  const dim3 sgrid(nblk, B, ksplit);
  if (masked && bf16_scores) coattn_scores_bf16_masked_kernel<<<sgrid, 256, 0, s>>>(sp, valid_u, valid_i);
  else if (masked) coattn_scores_masked_kernel<<<sgrid, 256, 0, s>>>(sp, valid_u, valid_i);
  else if (bf16_scores) coattn_scores_bf16_kernel<<<sgrid, 256, 0, s>>>(sp);
  else coattn_scores_kernel<<<sgrid, 256, 0, s>>>(sp);
  UMPR_LAUNCH_CHECK("coattn_scores");
  FinishParams fp{Gu, Gi, W.cpart, W.apart, nblk, W.rpart, W.arpart, ksplit, rowmax, argrow, colmax, argcol, soft_u, soft_i, atte_u, ld_u, atte_i, ld_i, SL};
  if (masked) coattn_finish_masked_kernel<<<dim3(B, 2), 1024, SL * sizeof(float), s>>>(fp);
  else coattn_finish_kernel<<<dim3(B, 2), 1024, SL * sizeof(float), s>>>(fp);
  UMPR_LAUNCH_CHECK("coattn_finish");
  return 0;
}

size_t umpr_coattn_bwd_ws_bytes(int B, int SL) { return coattn_bwd_ws(nullptr, B, SL).bytes; }

int umpr_coattn_bwd_impl(const float* Gu, const float* Gi, const float* M, const float* T, const float* soft_u,
                         const float* soft_i, const float* colmax, const int* argcol, const float* rowmax,
                         const int* argrow, const float* d_atte_u, long ld_du, const float* d_atte_i, long ld_di,
                         const float* d_soft_u, const float* d_soft_i, int B, int SL, float* dGu, float* dGi, float* dM,
                         int accumulate, float* ws, size_t ws_bytes, bool gemm_b16, hipStream_t s) {
  const CoattnBwdWs W = coattn_bwd_ws(ws, B, SL);
  UMPR_REQUIRE(ws_bytes >= W.bytes, "coattn_bwd: workspace too small");
  float *dSc = W.dSc, *dSr = W.dSr, *dT = W.dT;
  BwdPrepParams pp{Gu, Gi, d_atte_u, ld_du, d_atte_i, ld_di, d_soft_u, d_soft_i, soft_u, soft_i, colmax, rowmax, dSc, dSr, SL};
  coattn_bwd_prep_kernel<<<dim3(B, 2), 1024, SL * sizeof(float), s>>>(pp);
  UMPR_LAUNCH_CHECK("coattn_bwd_prep");
  BwdRowsParams rp{Gu, T, soft_u, soft_i, d_atte_u, ld_du, d_atte_i, ld_di, dSc, dSr, argcol, argrow, dGu, dT, dGi, SL, accumulate};
  coattn_bwd_rows_kernel<<<dim3(cdiv(SL, 16), B), 256, 4 * SL * sizeof(float), s>>>(rp);
  UMPR_LAUNCH_CHECK("coattn_bwd_rows");
  // dG_i += dT M^T
  UmprGemm g;
  g.A = dT; g.lda = D; g.B = M; g.ldb = D; g.transB = true; g.C = dGi; g.ldc = D; g.M = B * SL; g.N = D; g.K = D;
  g.accumulate = true; g.b16 = gemm_b16;
  if (int rc = umpr_gemm(g, s)) return rc;
  // dM = G_i^T dT   (K = B*SL, split-K)
  UmprGemm h;
  h.A = Gi; h.lda = D; h.transA = true; h.B = dT; h.ldb = D; h.C = dM; h.ldc = D; h.M = D; h.N = D; h.K = B * SL;
  h.split_k = 0; h.ws = W.slab; h.ws_bytes = W.slab_bytes; h.b16 = gemm_b16;
  return umpr_gemm(h, s);
}
